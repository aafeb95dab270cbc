// The frontier sweeps of class_sweep.hpp, class_sweep_cut.hpp and class_sweep_tiled.hpp under a weight per (syndrome, qubit): erasures -- every shot
// has its own erased qubits, which carry a uniform Pauli --, inhomogeneous noise, any per-shot prior.  The plans, the op streams, the holds, the
// segments and the launch groups are the siblings', unchanged; a CLOSE names its qubit (op[3]), and the one difference is that the four weights it
// multiplies by come from a table instead of four numbers shared by all qubits.
//
// THE TABLE.  The caller's wq is double[wq_rows][nq][4], the weights of I, X, Y, Z at every cell of the state layout; wq_rows is 1 -- one table for
// every syndrome -- or N -- row s belongs to syndrome s.  Host and device read it in (x, z) order I, X, Z, Y (site_rows_xz), as the siblings read
// their four weights: double[rows][nq][4], 32 bytes per qubit.  The weights of the CLOSE of qubit q in syndrome s are at
//     ((per_syndrome ? s : 0) * nq + q) * 4.
// The device holds the rows of one launch group at a time (s counts within the group), or the one table once: nothing grows with N.
//
// WEIGHTS are finite and >= 0.  Zero is allowed -- off an erased set the pure-erasure limit is (1, 0, 0, 0) -- and for weights <= 1 the arithmetic stays finite:
// copies, multiplies and adds of finite non-negative numbers.  Weights above 1 are accepted and can take a class weight to inf; small ones take it
// into the subnormals or to 0.  Z is returned as IEEE gives it, and qecmc.exact.law_from_class_weights judges it where it is normalised.  A qubit whose four weights are all zero makes every class weight zero and is refused
// by name.  Only the rows of qubits some CLOSE names are read or validated: a cell that holds no qubit (the planar code's unused cells) may hold
// anything.
//
// ARITHMETIC.  Every entry sees its sibling's sequence of copies, single multiplies and single adds, so each twin here agrees with its kernel
// (class_sweep_site.hip) bit for bit, and with constant rows each gives its uniform sibling's bits.
//
// Refused, before a device is looked for: what the sibling refuses, with its code and message; QECMC_ERR_INVALID for a wq_rows that is neither 1
// nor N (N > 0), for a weight that is negative, NaN or infinite and for a qubit with four zero weights.
#pragma once
#include "class_sweep_tiled.hpp"

namespace qecmc {
namespace sweep {

// the qubits some CLOSE of a four-word op stream names (the narrow and the wide encoding agree on the kind and on word 3)
inline std::vector<char> closed_qubits(const std::vector<uint32_t> &ops, int nq)
{
    std::vector<char> named((size_t)nq, 0);
    for (size_t o = 0; o + 3 < ops.size(); o += 4)
        if ((ops[o] & 15u) == kClose && ops[o + 3] < (uint32_t)nq) named[ops[o + 3]] = 1;
    return named;
}

inline Refusal check_site_rows(uint64_t N, uint64_t wq_rows)
{
    if (N > 0 && wq_rows != 1 && wq_rows != N)
        return refuse_params(QECMC_ERR_INVALID, "wq_rows=%llu: the site weights are one table (1) or one per syndrome (N=%llu)", (unsigned long long)wq_rows, (unsigned long long)N);
    return {};
}

// wq double[rows][nq][4] (I, X, Y, Z): finite and >= 0, not all zero, at every qubit `named` marks
inline Refusal check_site_weights(const double *wq, uint64_t rows, int nq, const std::vector<char> &named)
{
    static const char *const pauli = "IXYZ";
    for (uint64_t r = 0; r < rows; ++r)
        for (int q = 0; q < nq; ++q) {
            if (!named[(size_t)q]) continue;
            const double *w = wq + (r * (uint64_t)nq + (uint64_t)q) * 4u;
            bool any = false;
            for (int i = 0; i < 4; ++i) {
                if (!(w[i] >= 0.0) || !std::isfinite(w[i]))
                    return refuse_params(QECMC_ERR_INVALID, "wq[row %llu][qubit %d][%c]=%g: the site weights are finite and >= 0", (unsigned long long)r, q, pauli[i], w[i]);
                any = any || w[i] > 0.0;
            }
            if (!any) return refuse_params(QECMC_ERR_INVALID, "wq[row %llu][qubit %d]: the four weights of a qubit are all zero, and so is every class weight", (unsigned long long)r, q);
        }
    return {};
}

// rows of wq in (x, z) order: out double[rows][nq][4] = I, X, Z, Y (weights_xz per qubit; cells that hold no qubit are copied as they are)
inline void site_rows_xz(const double *wq, uint64_t rows, int nq, double *out)
{
    for (uint64_t i = 0; i < rows * (uint64_t)nq; ++i) weights_xz(wq + i * 4u, out + i * 4u);
}

// sweep_one() with the weights of the CLOSE's qubit: wxz double[nq][4] in (x, z) order
inline double sweep_one_site(const Plan &p, const uint32_t *rep, const double *wxz, double *A)
{
    A[0] = 1.0;
    host_ops(p.ops.data(), p.n_ops, rep, A, [&](double a, uint32_t q, uint32_t idx) { return a * wxz[(size_t)q * 4u + idx]; }, [](double a, double b) { return a + b; },
             NoDecisions{});
    return A[0] * p.scale;
}

// sweep_one_wide() with the weights of the CLOSE's qubit, unscaled
inline double sweep_one_wide_site(const TiledPlan &tp, const uint32_t *rep, const double *wxz, double *A)
{
    A[0] = 1.0;
    host_ops_wide(tp.ops.data(), tp.plan.n_ops, rep, A, [&](double a, uint32_t q, uint32_t idx) { return a * wxz[(size_t)q * 4u + idx]; },
                  [](double a, double b) { return a + b; });
    return A[0];
}

// The twins.  chains uint8[N][nq], wq double[wq_rows][nq][4] (I, X, Y, Z), wq_rows 1 or N -> Z double[N][ncls]; cls int32[N] (nullable).
inline void sweep_site_host(const Plan &p, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, double *Z, int32_t *cls)
{
    const size_t row = (size_t)p.nq * 4u;
    std::vector<double> wxz(row);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    std::vector<double> A((size_t)1 << p.width);
    for (uint64_t s = 0; s < N; ++s) {
        if (s == 0 || wq_rows != 1) site_rows_xz(wq + (wq_rows == 1 ? 0u : s) * row, 1, p.nq, wxz.data());
        const int a = class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        for (int c = 0; c < p.ncls; ++c) Z[s * (uint64_t)p.ncls + c] = sweep_one_site(p, &reps[(size_t)c * p.W], wxz.data(), A.data());
    }
}

// sweep_cut_host()'s sequence: the partial of every assignment of the held generators, then cut_reduce()
inline void sweep_cut_site_host(const CutPlan &cp, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, double *Z, int32_t *cls, unsigned threads = 0)
{
    const Plan &p = cp.plan;
    Plan unscaled = p;
    unscaled.scale = 1.0;                                                       // (A[0] * 1.0 is A[0])
    const uint32_t n_h = 1u << cp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = host_threads(threads, n_work, n_work, cp.n_held == 0);
    const size_t row = (size_t)p.nq * 4u;
    std::vector<double> wxz(row), P((size_t)n_work);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    for (uint64_t s = 0; s < N; ++s) {
        if (s == 0 || wq_rows != 1) site_rows_xz(wq + (wq_rows == 1 ? 0u : s) * row, 1, p.nq, wxz.data());
        const int a = class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        host_partials(n_work, threads, p.width, p.W, P.data(), [&](uint32_t i, uint32_t *rep, double *A) {
            cut_representative(cp, &reps[(size_t)(i >> cp.n_held) * p.W], i & (n_h - 1u), rep);
            return sweep_one_site(unscaled, rep, wxz.data(), A);
        });
        for (int c = 0; c < p.ncls; ++c) Z[s * (uint64_t)p.ncls + c] = cut_reduce(&P[(size_t)c << cp.n_held], cp.n_held, p.scale);
    }
}

// sweep_tiled_host()'s sequence: a plain loop over the wide stream per unit, then cut_reduce()
inline void sweep_tiled_site_host(const TiledPlan &tp, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, double *Z, int32_t *cls, unsigned threads = 0)
{
    const Plan &p = tp.plan;
    const uint32_t n_h = 1u << tp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = host_threads(threads, n_work, tiled_pass_units(p.width), p.width < 12);
    const size_t row = (size_t)p.nq * 4u;
    std::vector<double> wxz(row), P((size_t)n_work);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    for (uint64_t s = 0; s < N; ++s) {
        if (s == 0 || wq_rows != 1) site_rows_xz(wq + (wq_rows == 1 ? 0u : s) * row, 1, p.nq, wxz.data());
        const int a = class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        host_partials(n_work, threads, p.width, p.W, P.data(), [&](uint32_t i, uint32_t *rep, double *A) {
            tiled_representative(tp, &reps[(size_t)(i >> tp.n_held) * p.W], i & (n_h - 1u), rep);
            return sweep_one_wide_site(tp, rep, wxz.data(), A);
        });
        for (int c = 0; c < p.ncls; ++c) Z[s * (uint64_t)p.ncls + c] = cut_reduce(&P[(size_t)c << tp.n_held], tp.n_held, p.scale);
    }
}

}  // namespace sweep

// class_sweep_site.hip: all pointers are device pointers, as the siblings take them; wq double[per_syndrome ? S : 1][nq][4] in (x, z) order, rows of
// 32 bytes, 32-byte aligned.  S counts the syndromes of the launch group and the rows of wq with it.
struct SweepSiteArgs {
    uint32_t S;
    int ncls, W, width, n_ops, n_held, nq, per_syndrome;
    double scale;
};
hipError_t launch_class_sweep_site(const SweepSiteArgs &a, const uint32_t *ops, const uint32_t *reps, const double *wq, double *z, hipStream_t stream);
hipError_t class_sweep_cut_site_allow_lds(int width);  // class_sweep_cut_allow_lds() for k_class_sweep_cut_site
hipError_t launch_class_sweep_cut_site(const SweepSiteArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *P, double *z,
                                       hipStream_t stream);
// k_class_sweep_cut_site alone: the unscaled partials, left as they are (class_sample.hip picks an assignment from them)
hipError_t launch_class_sweep_cut_site_partials(const SweepSiteArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *P,
                                                hipStream_t stream);
struct SweepTiledSiteArgs {
    uint32_t unit_first, units;        // as SweepTiledArgs, without the four weights
    int W, n_held, state_bits, tile_width;
    uint32_t op_first, op_count, tile, fixed_live, local_in, local_out, n_tiles, first, last;
    int ncls, nq, per_syndrome;
};
hipError_t launch_class_sweep_tiled_site(const sweep::TiledPlan &tp, int per_syndrome, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                         const uint32_t *reps, const double *wq, double *work, double *P, hipStream_t stream);

}  // namespace qecmc
