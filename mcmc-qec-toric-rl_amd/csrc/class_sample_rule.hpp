// What the two routes of the exact chain sampler share -- class_sample.hpp on the cut plans, class_sample_tiled.hpp on the plans tiled over HBM --: the
// sub-stream and the bits of a uniform, the 16-byte pair a FORGET records, the floor of the law, the checks both sides make in one order and in one
// wording, the running-sum pick and the decision of the walk.  THE RULE itself is stated in class_sample.hpp; nothing here knows a plan's layout.
#pragma once
#include "class_sweep_site.hpp"

#include <cstring>

namespace qecmc {
namespace sample {

constexpr uint32_t kSubSample = 0x53u;                       // the sub-stream of every draw here (DESIGN.md "RNG addressing"): no sampler uses it
// The least class weight (every-class mode) or row total (posterior mode) a draw is made from: qecmc.exact.LAW_FLOOR, 2^-960 compared at half of it so
// that an exact 2^-960 is never refused on account of the sweep's own relative error.  Below it the record's pairs are multiples of 2^-1074 rounded by
// up to 2^-1075 each, and on / s is no longer the branch's probability to 1e-12 (DESIGN.md 4.1s "Range")
constexpr double kSampleFloor = 0x1p-961;

struct PairRecord { double on, s; };
static_assert(sizeof(PairRecord) == 16, "one 16-byte store per lane");

inline Refusal named(const char *name, Refusal r)
{
    if (r.code) r.msg = std::string(name) + ": " + r.msg;
    return r;
}

// ---------------------------------------------------------------- the checks both sides make, in this order
inline Refusal check_sample_args(const char *name, uint64_t N, uint64_t K, uint32_t first_syndrome, int mode)
{
    if (N > 0xFFFFFFFFull || (uint64_t)first_syndrome + N > 0x100000000ull)
        return named(name, refuse_params(QECMC_ERR_INVALID, "N=%llu syndromes from first_syndrome=%u exceed 32 bits", (unsigned long long)N, first_syndrome));
    if (K == 0 || K > 0xFFFFFFFFull) return named(name, refuse_params(QECMC_ERR_INVALID, "K=%llu: the samples per syndrome are 1 .. 2^32 - 1", (unsigned long long)K));
    if (mode != 0 && mode != 1) return named(name, refuse_params(QECMC_ERR_INVALID, "mode=%d: 0 draws chains of every class, 1 draws the class first", mode));
    return {};
}

// the four weights: finite and >= 0, not all zero -- a zero is allowed here, and a class it empties is refused by name once Z is known
inline Refusal check_sample_weights(const char *name, const double *w)
{
    bool any = false;
    for (int i = 0; i < 4; ++i) {
        if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return named(name, refuse_params(QECMC_ERR_INVALID, "w[%d]=%g: the weights of I, X, Y and Z are finite and >= 0", i, w[i]));
        any = any || w[i] > 0.0;
    }
    if (!any) return named(name, refuse_params(QECMC_ERR_INVALID, "the four weights are all zero, and so is every class weight"));
    return {};
}

inline Refusal check_sample_site(const char *name, uint64_t N, const double *wq, uint64_t wq_rows, const sweep::Plan &p)
{
    if (const Refusal r = sweep::check_site_rows(N, wq_rows); r.code) return named(name, r);
    return N ? named(name, sweep::check_site_weights(wq, wq_rows, p.nq, sweep::closed_qubits(p.ops, p.nq))) : Refusal{};
}

// Z double[ncls] of input row `row`: every-class mode needs every class, posterior mode the row's total (the running sum the class is drawn from)
inline Refusal check_sample_z(const char *name, uint64_t row, const double *Z, int ncls, int mode)
{
    if (mode == 0) {
        for (int c = 0; c < ncls; ++c)
            if (!(Z[c] > 0.0) || !std::isfinite(Z[c]))
                return named(name, refuse_params(QECMC_ERR_INVALID, "row %llu, class %d: the class weight is %g -- a class whose weight is 0 or not finite has no chain to draw",
                                                 (unsigned long long)row, c, Z[c]));
            else if (Z[c] < kSampleFloor)
                return named(name, refuse_params(QECMC_ERR_INVALID, "row %llu, class %d: the class weight is %g, below 2^-960 = %g: it underflows into the subnormal range of "
                                                 "float64, where the ratios of the record are rounded away, and the chains of that class cannot be drawn by their law",
                                                 (unsigned long long)row, c, Z[c], 2.0 * kSampleFloor));
        return {};
    }
    double total = Z[0];
    for (int c = 1; c < ncls; ++c) total = total + Z[c];
    if (!(total > 0.0) || !std::isfinite(total))
        return named(name, refuse_params(QECMC_ERR_INVALID, "row %llu: the class weights total %g -- a row whose total is 0 or not finite has no class to draw", (unsigned long long)row, total));
    if (total < kSampleFloor)
        return named(name, refuse_params(QECMC_ERR_INVALID, "row %llu: the class weights total %g, below 2^-960 = %g: they underflow into the subnormal range of float64, where "
                                         "their ratios are rounded away, and the posterior of that row cannot be drawn by its law", (unsigned long long)row, total,
                                         2.0 * kSampleFloor));
    return {};
}

// ---------------------------------------------------------------- what host and device share: the uniform's bits
__host__ __device__ inline double u53_of(uint32_t hi, uint32_t lo) { return (double)(((uint64_t)hi << 21) | (uint64_t)(lo >> 11)) * 0x1p-53; }

// Philox4x32-10 at the address of philox.hpp's philox_block -- counter (index[31:0], index[47:32] | sub << 16, syndrome, stream), key = seed --, written
// here for the host alone: the kernels draw through philox.hpp
inline double draw_u53(uint64_t k, uint32_t block, uint32_t j, uint32_t syndrome, uint32_t stream, uint64_t seed)
{
    const uint64_t index = (k << 16) | (uint64_t)block;
    uint32_t c[4] = {(uint32_t)index, (uint32_t)((index >> 32) & 0xFFFFu) | (kSubSample << 16), syndrome, stream}, key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const uint32_t n[4] = {(uint32_t)(p1 >> 32) ^ c[1] ^ key0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c[3] ^ key1, (uint32_t)p0};
        std::memcpy(c, n, sizeof n);
        key0 += 0x9E3779B9u; key1 += 0xBB67AE85u;
    }
    return u53_of(c[2u * j], c[2u * j + 1u]);
}

// step 2, and the class of posterior mode: the lowest index whose running sum passes u * (the last running sum), or has reached it -- where the product
// rounds up to the last sum (a subnormal one) no sum passes it, and the first to reach the last is an entry > 0, which the last index need not be
inline uint32_t pick_running(const double *v, uint32_t n, double u)
{
    double last = v[0];
    for (uint32_t i = 1; i < n; ++i) last = last + v[i];
    const double t = u * last;
    double run = v[0];
    uint32_t i = 0;
    while (!(t < run || run == last) && i + 1u < n) { ++i; run = run + v[i]; }
    return i;
}

// step 4's decision at a FORGET whose record holds (on, s) under the uniform u: the generator is taken iff u * s < on, or the branch is forced -- one
// multiply and two compares; where s is subnormal u * s may round back up to s, and the second compare alone keeps a forced branch
__host__ __device__ inline bool take_branch(double u, double on, double s) { return u * s < on || on == s; }

}  // namespace sample
}  // namespace qecmc
