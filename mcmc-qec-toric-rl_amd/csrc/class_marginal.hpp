// Exact per-qubit marginals of every class: the sum-product cut sweep of class_sweep_cut.hpp run forward with a record of the state vector after every
// CLOSE, and a second state vector swept backward over the same stream -- forward filtering and a backward sum, where class_sample.hpp is forward
// filtering and backward sampling.  For syndrome s, class c and qubit q the result is
//     weights[s][c][q][P] = the sum of w(chain) over the chains of class c with the syndrome of chain s that carry Pauli P at q,
// so that weights / Z_c is P(qubit q carries P | syndrome, class), and the sum over the classes, over the sum of the Z_c, the posterior's.
//
// THE RULE, for syndrome s, class c, with the cut plan cp of (code, L, lds_width), the class representative rep_c and the factors w (four per call, or
// a site table).  One JOB is one (s, c, h), h an assignment of the held generators; its representative is cut_representative(cp, rep_c, h).
//     1. FORWARD   A[0] = 1, the op loop of class_sweep_ops.hpp; after CLOSE number ci (its ordinal in the stream) every live f keeps A[f]:
//                      fwd[ci][f],  f < 2^width,  8 bytes.   Dead f keep nothing and are never read.  The job's partial is P[h] = A[0] after the last op.
//     2. BACKWARD  B[0] = 1 over the same slots, the ops in reverse:
//                      FORGET(slot)   B[f | bit] = B[f]              for live f under the mask the FORGET has after it (a copy)
//                      INTRO(slot)    B[f] = B[f] + B[f | bit]       for live f under the mask the INTRO has before it
//                      CLOSE(q), ci   d[f] = fwd[ci][f] * B[f],  then  B[f] = B[f] * w_q[idx(f)],  for live f; idx(f) as the forward CLOSE forms it.
//     3. FOLD      the slice (job, ci) is folded by kFoldLanes = 64 lanes.  For each x in 0 .. 3 lane l holds v_x[l], +0.0 at first, and adds the d[f]
//                  of the live f with f mod 64 == l and idx(f) == x in ascending f: v_x[l] = v_x[l] + d[f].  Then, for m = 32, 16, 8, 4, 2, 1 in this
//                  order, every lane at once: v_x[l] = v_x[l] + v_x[l ^ m].  M_h[ci][x] = v_x[0].  Four sums per slice.
//     4. HELD      M_c[ci][x] = cut_reduce over h of M_h[ci][x] -- for j = 0 .. n_held - 1 ascending, M[h] = M[h] + M[h | 1 << j] over the h whose bits
//                  0 .. j are clear -- times plan.scale: the adds Z_c gets from the partials, in the same order.  Z_c = cut_reduce of P, as ever.
//     5. RESULT    weights[s][c][q][P] = M_c[ci of q][pauli_to_xz(P)]: idx is the (x, z) of the Pauli that sits on the qubit.  A cell no CLOSE names
//                  (the planar code's unused cells) gets Z_c at the representative's byte and 0 elsewhere.
// The order of every add is a function of the plan and of kFoldLanes alone: not of N, the launch grouping, the number of workgroups or the threads
// of a workgroup (the lanes of the fold are the rule's 64, whatever walks them).  Every quantity is a product or a sum of non-negative numbers: no
// subtraction, no division; a weight of 0 gives exact zeros.  The sum over x of M_h[ci][x] is P[h] up to rounding, at every ci.
// The kernels (class_marginal.hip) and the twin below (marginal_host) are written apart, both without floating-point contraction, and agree bit for bit.
//
// MEMORY.  The forward record of a job is n_close * 2^width * 8 bytes (15.1 MiB at rotated L = 11, 3.1 MiB at toric L = 5 under width 13);
// marginal_launch_group bounds the records of one launch by kMarginalWorkspaceBytes, and the syndromes of one group so that the M_h of the group
// stay within kMarginalFoldBytes and its partials within a sweep launch, whatever N.
//
// Refused, before a device is looked for, under the entry point's name, in this order: a NULL buffer; N past 32 bits; a weight that is negative or
// not finite, four zero weights (single zeros are allowed); what build_cut_plan refuses, with its code; the site-table checks of check_sample_site.
#pragma once
#include "class_sample.hpp"          // named(), check_sample_weights, check_sample_site, Factors

namespace qecmc {
namespace marginal {

constexpr uint32_t kFoldLanes = 64;                            // the lanes of THE RULE's fold: a constant of the rule, not of the launch
constexpr uint64_t kMarginalWorkspaceBytes = 512ull << 20;     // the forward records of one launch
constexpr uint64_t kMarginalFoldBytes = 64ull << 20;           // M_h of one group of syndromes: [jobs][n_close][4] doubles

struct MarginalPlan {
    sweep::CutPlan cut;                 // refusal: cut.plan.refusal, prefixed with the entry point's name
    int n_close = 0;
    std::vector<uint32_t> close_op;     // [n_close]: the op index of CLOSE ci, in stream order
    std::vector<uint32_t> close_qubit;  // [n_close]: its qubit
    std::vector<int32_t> close_of;      // [nq]: the ordinal of the CLOSE that names the cell, -1: none does
};

// build_cut_plan -- the sum-product plan, unchanged -- with its refusals under `name`, and where its CLOSEs are
inline MarginalPlan build_marginal_plan(int code, int L, int lds_width, const char *name = "qecmc_class_marginals")
{
    MarginalPlan mp;
    mp.cut = sweep::build_cut_plan(code, L, lds_width);
    sweep::Plan &p = mp.cut.plan;
    if (p.refusal.code) { p.refusal = sample::named(name, p.refusal); return mp; }
    mp.close_of.assign((size_t)p.nq, -1);
    bool once = true;
    for (int o = 0; o < p.n_ops; ++o) {
        if ((p.ops[(size_t)o * sweep::kOpWords] & 15u) != sweep::kClose) continue;
        const uint32_t q = p.ops[(size_t)o * sweep::kOpWords + 3];
        if (q >= (uint32_t)p.nq || mp.close_of[q] >= 0) { once = false; break; }
        mp.close_of[q] = (int32_t)mp.close_op.size();
        mp.close_op.push_back((uint32_t)o);
        mp.close_qubit.push_back(q);
    }
    mp.n_close = (int)mp.close_op.size();
    if (!once || mp.n_close < 1)
        p.refusal = sample::named(name, refuse_params(QECMC_ERR_UNSUPPORTED, "internal: the stream of code %d at L=%d does not close every qubit once", code, L));
    return mp;
}

// the forward record of one job, in entries and in bytes; M_h of one job in doubles
inline uint64_t marginal_entries_per_job(int n_close, int width) { return (uint64_t)n_close << width; }
inline uint64_t marginal_bytes_per_job(const MarginalPlan &mp) { return marginal_entries_per_job(mp.n_close, mp.cut.plan.width) * sizeof(double); }
inline uint64_t marginal_fold_per_job(int n_close) { return (uint64_t)n_close * 4u; }

// How a call becomes launches.  syndromes: cut_launch_group -- the partials of a group are one sweep launch's --, and few enough that the M_h of the
// group's jobs stay within kMarginalFoldBytes -- or one syndrome, where one alone takes more: 2^16 jobs of 50 CLOSEs, 100 MiB, is the most a plan
// can ask for --; jobs: the forward records of one forward / backward / fold launch, within kMarginalWorkspaceBytes and kCutGridMax (never 0: the
// largest accepted record is 15.1 MiB).  N enters through cut_launch_group's min(N, .) alone.
struct LaunchGroup { uint32_t syndromes, jobs; };
inline LaunchGroup marginal_launch_group(uint64_t N, int ncls, int n_held, int n_close, uint64_t bytes_per_job)
{
    LaunchGroup g;
    g.syndromes = sweep::cut_launch_group(N, ncls, n_held);
    const uint64_t per_syndrome = ((uint64_t)ncls << n_held) * marginal_fold_per_job(n_close) * sizeof(double);
    uint64_t fit = kMarginalFoldBytes / (per_syndrome ? per_syndrome : 1ull);
    if (fit < 1ull) fit = 1ull;
    if (fit < g.syndromes) g.syndromes = (uint32_t)fit;
    uint64_t cap = kMarginalWorkspaceBytes / (bytes_per_job ? bytes_per_job : 1ull);
    if (cap < 1ull) cap = 1ull;
    if (cap > sweep::kCutGridMax) cap = sweep::kCutGridMax;
    const uint64_t all = (uint64_t)g.syndromes * ((uint64_t)ncls << n_held);
    g.jobs = (uint32_t)(all < cap ? all : cap);
    return g;
}

// ---------------------------------------------------------------- the checks both sides make, in this order (after the NULL buffers)
inline Refusal check_marginal_args(const char *name, uint64_t N)
{
    if (N > 0xFFFFFFFFull) return sample::named(name, refuse_params(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N));
    return {};
}
inline Refusal check_marginal_weights(const char *name, const double *w) { return sample::check_sample_weights(name, w); }
inline Refusal check_marginal_site(const char *name, uint64_t N, const double *wq, uint64_t wq_rows, const sweep::Plan &p) { return sample::check_sample_site(name, N, wq, wq_rows, p); }

// ---------------------------------------------------------------- the twin
// step 1 of one job: host_ops one op at a time, the live entries kept after every CLOSE.  A: 2^width doubles, fwd: marginal_entries_per_job doubles,
// both dirty allowed -> the unscaled partial
inline double forward_one(const MarginalPlan &mp, const uint32_t *rep, const sample::Factors &fc, double *A, double *fwd)
{
    const sweep::Plan &p = mp.cut.plan;
    A[0] = 1.0;
    size_t ci = 0;
    for (int o = 0; o < p.n_ops; ++o) {
        const uint32_t *op = p.ops.data() + (size_t)o * sweep::kOpWords;
        sweep::host_ops(op, 1, rep, A, [&](double a, uint32_t q, uint32_t idx) { return a * fc.tab[(size_t)q * fc.stride + idx]; }, [](double a, double b) { return a + b; },
                        sweep::NoDecisions{});
        if ((op[0] & 15u) != sweep::kClose) continue;
        const uint32_t top = (op[0] >> 12) & 31u, mask = op[1];
        double *keep = fwd + (ci++ << p.width);
        for (uint32_t f = 0; f < (1u << top); ++f)
            if (!(f & ~mask)) keep[f] = A[f];
    }
    return A[0];
}

// steps 2 and 3 of one job: the reverse loop, with the fold of every slice as THE RULE orders it.  B: 2^width doubles, dirty allowed;
// fwd: forward_one's, left as it was; Mh double[n_close][4] in (x, z) order
inline void backward_one(const MarginalPlan &mp, const uint32_t *rep, const sample::Factors &fc, double *B, const double *fwd, double *Mh)
{
    using namespace sweep;
    const Plan &p = mp.cut.plan;
    B[0] = 1.0;
    size_t ci = (size_t)mp.n_close;
    for (int o = p.n_ops - 1; o >= 0; --o) {
        const uint32_t *op = p.ops.data() + (size_t)o * kOpWords;
        const uint32_t kind = op[0] & 15u, slot = (op[0] >> 4) & 15u, top = (op[0] >> 12) & 31u, mask = op[1], bit = 1u << slot;
        if (kind == kClose) {
            --ci;
            const uint32_t q = op[3], cq = pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
            const double *kept = fwd + (ci << p.width);
            double v[4][kFoldLanes];
            for (int x = 0; x < 4; ++x)
                for (uint32_t l = 0; l < kFoldLanes; ++l) v[x][l] = 0.0;
            for (uint32_t f = 0; f < (1u << top); ++f) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (op[2] >> (8 * j)) & 0xFFu;
                    if ((f >> (pr & 15u)) & 1u) idx ^= pr >> 4;
                }
                const double d = kept[f] * B[f];
                v[idx][f % kFoldLanes] = v[idx][f % kFoldLanes] + d;
                B[f] = B[f] * fc.tab[(size_t)q * fc.stride + idx];
            }
            for (int x = 0; x < 4; ++x) {
                for (uint32_t m = kFoldLanes / 2u; m >= 1u; m >>= 1) {
                    double next[kFoldLanes];
                    for (uint32_t l = 0; l < kFoldLanes; ++l) next[l] = v[x][l] + v[x][l ^ m];
                    for (uint32_t l = 0; l < kFoldLanes; ++l) v[x][l] = next[l];
                }
                Mh[ci * 4u + (size_t)x] = v[x][0];
            }
            continue;
        }
        for (uint32_t h = 0; h < (1u << (top - 1u)); ++h) {
            const uint32_t f = insert_zero(h, slot);
            if (f & ~mask) continue;
            if (kind == kForget) B[f | bit] = B[f];
            else B[f] = B[f] + B[f | bit];
        }
    }
}

// The twin.  chains uint8[N][nq]; w4[4] (I, X, Y, Z), or wq double[wq_rows][nq][4] where w4 is NULL -> weights_out double[N][ncls][nq][4] (I, X, Y, Z),
// z_out double[N][ncls], class_out int32[N] (nullable).  The arguments are checked by the caller.  The jobs of one syndrome are spread over host
// threads; every job is formed alone and every sum in the rule's order, whatever their number.
inline void marginal_host(const MarginalPlan &mp, uint64_t N, const uint8_t *chains, const double *w4, const double *wq, uint64_t wq_rows, double *weights_out, double *z_out,
                          int32_t *class_out, unsigned threads = 0)
{
    const sweep::CutPlan &cp = mp.cut;
    const sweep::Plan &p = cp.plan;
    const uint32_t n_h = 1u << cp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = sweep::host_threads(threads, n_work, n_work, false);
    const size_t row = (size_t)p.nq * 4u, per_job = (size_t)marginal_fold_per_job(mp.n_close);
    std::vector<double> wxz(w4 ? 4u : row), P((size_t)n_work), Mh((size_t)n_work * per_job), fold((size_t)n_h);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    if (w4) sweep::weights_xz(w4, wxz.data());
    const sample::Factors fc{wxz.data(), w4 ? 0u : 4u};
    auto work = [&](unsigned t) {
        std::vector<double> A((size_t)1 << p.width), B((size_t)1 << p.width), fwd((size_t)marginal_entries_per_job(mp.n_close, p.width));
        std::vector<uint32_t> rep((size_t)p.W);
        for (uint32_t i = t; i < n_work; i += threads) {
            sweep::cut_representative(cp, &reps[(size_t)(i >> cp.n_held) * p.W], i & (n_h - 1u), rep.data());
            P[i] = forward_one(mp, rep.data(), fc, A.data(), fwd.data());
            backward_one(mp, rep.data(), fc, B.data(), fwd.data(), &Mh[(size_t)i * per_job]);
        }
    };
    for (uint64_t s = 0; s < N; ++s) {
        if (!w4 && (s == 0 || wq_rows != 1)) sweep::site_rows_xz(wq + (wq_rows == 1 ? 0u : s) * row, 1, p.nq, wxz.data());
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (class_out) class_out[s] = a;
        if (threads <= 1u) work(0);
        else {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < threads; ++t) pool.emplace_back(work, t);
            for (std::thread &t : pool) t.join();
        }
        for (int c = 0; c < p.ncls; ++c) {
            const size_t first = (size_t)c << cp.n_held;
            std::memcpy(fold.data(), &P[first], (size_t)n_h * sizeof(double));
            const double Zc = z_out[s * (uint64_t)p.ncls + c] = sweep::cut_reduce(fold.data(), cp.n_held, p.scale);
            double *out = weights_out + (s * (uint64_t)p.ncls + (uint64_t)c) * row;
            for (int q = 0; q < p.nq; ++q) {
                const int32_t ci = mp.close_of[(size_t)q];
                const uint32_t here = (reps[(size_t)c * p.W + (size_t)(q >> 4)] >> ((q & 15) * 2)) & 3u;
                for (uint32_t pauli = 0; pauli < 4u; ++pauli) {
                    if (ci < 0) { out[(size_t)q * 4u + pauli] = pauli == here ? Zc : 0.0; continue; }
                    for (uint32_t h = 0; h < n_h; ++h) fold[h] = Mh[(first + h) * per_job + (size_t)ci * 4u + sweep::pauli_to_xz(pauli)];
                    out[(size_t)q * 4u + pauli] = sweep::cut_reduce(fold.data(), cp.n_held, p.scale);
                }
            }
        }
    }
}

}  // namespace marginal

// class_marginal.hip: all pointers are device pointers.  ops, held and reps as class_sweep_cut.hip takes them; close_op uint32[n_close], close_of
// int32[nq].  The jobs of a group of S syndromes are numbered job = ((s * ncls + c) << n_held) + h, as k_class_sweep_cut numbers its workgroups;
// a launch takes jobs [job0, job0 + jobs).
struct MarginalArgs {
    uint32_t S, job0, jobs;
    int ncls, W, width, n_ops, n_held, n_close, nq, per_syndrome;
    double wxz[4], scale;
};
hipError_t class_marginal_allow_lds(int width, int site);  // hipSuccess: the forward and backward kernels (uniform / site) can be launched at this width
// k_class_marginal_fwd / _fwd_site: job job0 + b sweeps forward, keeps record b of fwd -- double[jobs][n_close][2^width], scratch, dirty allowed -- and
// writes its unscaled partial P[job0 + b].  wq: NULL for the four weights of a.wxz, else double[per_syndrome ? S : 1][nq][4] in (x, z) order, 32-byte aligned
hipError_t launch_marginal_forward(const MarginalArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *fwd, double *P,
                                   hipStream_t stream);
// k_class_marginal_bwd / _bwd_site, after the forward kernel on the same stream: record b becomes d[f] in place
hipError_t launch_marginal_backward(const MarginalArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *fwd, hipStream_t stream);
// k_class_marginal_fold, after the backward kernel: Mh double[S * ncls << n_held][n_close][4] gets the rows of jobs [job0, job0 + jobs)
hipError_t launch_marginal_fold(const MarginalArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *close_op, const double *fwd, double *Mh,
                                hipStream_t stream);
// k_class_marginal_combine, after every fold of the group and after z double[S][ncls] is formed: Mh is folded over h in place, out double[S][ncls][nq][4]
hipError_t launch_marginal_combine(const MarginalArgs &a, const uint32_t *reps, const int32_t *close_of, double *Mh, const double *z, double *out, hipStream_t stream);

}  // namespace qecmc
