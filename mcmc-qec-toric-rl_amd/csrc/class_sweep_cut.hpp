// The frontier sweep of class_sweep.hpp past one LDS state vector, by cut-set conditioning.  Hold a set H of generators out of the elimination.  For
// every assignment h in {0,1}^|H| the held generators with their bit set in h are multiplied into the class representative -- an XOR on the packed
// words -- and the remaining generators are swept by an ordinary op stream over a narrower frontier.  Then
//     Z_c = 2^-(G - rank) * sum over h of Z_c(h)
// exactly: the sum over all subsets of the generator table, split by the subset's part in H.  One (class, syndrome) becomes 2^|H| workgroups, each
// with a state vector in LDS, and a sum of their partials in a fixed order.
//
// THE HOLD RULE (build_cut_plan): build the stream as build_plan orders it; while its peak exceeds lds_width, of the generators live at the FIRST op
// at which the peak is reached hold the one with the longest lifetime (FORGET position minus INTRO position in that stream), ties to the lowest table
// index, and build again.  A held generator has no INTRO and no FORGET and no CLOSE names it; a qubit touched by held generators only is closed with
// no pair.  Holding one generator narrows the peak by one at most, so a frontier more than kMaxHeld wider than lds_width is refused at once.
//
// ARITHMETIC: the partial P[h] is sweep_one()'s A[0] on the modified representative, unscaled.  The partials are summed as a FORGET on the held bits:
// for j = 0 .. n_held - 1 ascending, P[h] += P[h | 1 << j] over the h whose bits 0 .. j are clear; Z = P[0] * scale.  Kernels (class_sweep_cut.hip)
// and twin (sweep_cut_host) follow the same sequence, so they agree bit for bit; with nothing held the result is build_plan's, bit for bit.
//
// lds_width is 2 .. kCutMaxWidth (14: 128 KiB, which a launch opts in to); 0 is default_width().  Refused before a device is looked for: what
// build_plan refuses but the width; QECMC_ERR_INVALID for an lds_width out of range; QECMC_ERR_UNSUPPORTED where more than kMaxHeld generators would
// have to be held.
#pragma once
#include "class_sweep.hpp"

#include <mutex>

namespace qecmc {
namespace sweep {

constexpr int kMaxHeld = 12;                        // 4 096 workgroups per (class, syndrome) at most
constexpr uint32_t kCutLdsBudget = 128 * 1024;      // the dynamic-LDS window a launch may opt in to: one workgroup per CU of 160 KiB
constexpr uint32_t kCutGridMax = 1u << 16;          // workgroups of one launch of the sweep kernel

// what fits the LDS of one workgroup: the launch asks this function too
constexpr bool cut_fits(int width) { return width >= 1 && lds_carve(width).bytes != 0 && lds_carve(width).bytes <= kCutLdsBudget; }
constexpr int cut_max_width()
{
    int w = 0;
    while (cut_fits(w + 1)) ++w;
    return w;
}
constexpr int kCutMaxWidth = cut_max_width();       // 14
static_assert(kCutMaxWidth == 14 && kCutMaxWidth <= 15, "the op words keep a slot in 4 bits and the mask in 16");
// Threads of a sweep workgroup: kThreads, as k_class_sweep, up to width 12; QECMC_CUT_THREADS_W13 at width 13 (two workgroups share a CU) and
// QECMC_CUT_THREADS_W14 at width 14 (the state vector takes the CU alone) -- build-time switches for measuring them, DESIGN.md 4.1l has the figures
// the defaults come from.  The kernel strides by blockDim.x: the entries see the same operations whatever the number of lanes.
#ifndef QECMC_CUT_THREADS_W13
#define QECMC_CUT_THREADS_W13 1024
#endif
#ifndef QECMC_CUT_THREADS_W14
#define QECMC_CUT_THREADS_W14 1024
#endif
constexpr int kCutThreadsMax = 1024;
constexpr uint32_t cut_threads(int width) { return width >= 14 ? (uint32_t)(QECMC_CUT_THREADS_W14) : width == 13 ? (uint32_t)(QECMC_CUT_THREADS_W13) : (uint32_t)kThreads; }
static_assert(QECMC_CUT_THREADS_W13 >= 64 && QECMC_CUT_THREADS_W13 <= kCutThreadsMax && QECMC_CUT_THREADS_W13 % 64 == 0, "whole wavefronts within the launch bound");
static_assert(QECMC_CUT_THREADS_W14 >= 64 && QECMC_CUT_THREADS_W14 <= kCutThreadsMax && QECMC_CUT_THREADS_W14 % 64 == 0, "whole wavefronts within the launch bound");
// The width the toric code at L = 5 -- the one accepted shape that holds generators under either width -- is swept at by default: 13 (2^8 workgroups per
// class, two per CU) or 14 (2^7, one per CU).  Measured, 1 024 threads each: 28.9 ms against 35.0 ms for 16 syndromes.
constexpr int kDefaultHeldWidth = 13;

struct CutPlan {
    Plan plan;                         // the stream of the generators that are not held; width: its peak.  refusal: the cut plan's
    int lds_width = 0, full_width = 0, n_held = 0;
    std::vector<int> held;             // table indices, ascending
    std::vector<uint32_t> held_words;  // [n_held][W]: held generator j as packed state words, 2 bits per qubit
};

// lds_width = 0: kMaxWidth where nothing is held then; kCutMaxWidth where that holds nothing; kDefaultHeldWidth elsewhere
inline int default_width(int full_width) { return full_width <= kMaxWidth ? kMaxWidth : full_width <= kCutMaxWidth ? kCutMaxWidth : kDefaultHeldWidth; }

// the hold rule: of the generators live at the first op at which the stream reaches its peak, the one with the longest lifetime, ties to the lowest
// table index; -1: none is live there
inline int pick_hold(const Trace &tr, int n_gen)
{
    int pick = -1, longest = -1;
    for (int g = 0; g < n_gen; ++g) {
        if (tr.intro_at[(size_t)g] < 0 || tr.intro_at[(size_t)g] > tr.first_peak_op || tr.forget_at[(size_t)g] < tr.first_peak_op) continue;   // not live there
        const int life = tr.forget_at[(size_t)g] - tr.intro_at[(size_t)g];
        if (life > longest) { longest = life; pick = g; }
    }
    return pick;
}

// the held generators of a plan: their table indices, ascending, and each as packed state words [W], 2 bits per qubit
inline void held_generator_words(const correct::Table &ct, const std::vector<char> &held, std::vector<int> &index, std::vector<uint32_t> &words_out)
{
    for (int g = 0; g < ct.n_gen; ++g) {
        if (!held[(size_t)g]) continue;
        index.push_back(g);
        std::vector<uint32_t> words((size_t)ct.W, 0u);
        for (int i = 0; i < 4; ++i) {
            const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
            words[site >> 4] ^= pauli << ((site & 15u) * 2u);                   // (Pauli values XOR as the Pauli product)
        }
        words_out.insert(words_out.end(), words.begin(), words.end());
    }
}

inline CutPlan build_cut_plan(int code, int L, int lds_width)
{
    CutPlan cp;
    if (lds_width != 0 && (lds_width < 2 || lds_width > kCutMaxWidth)) {
        cp.plan.code = code; cp.plan.L = L;
        cp.plan.refusal = refuse_params(QECMC_ERR_INVALID, "lds_width=%d: the width of the state vector in LDS is 2 .. %d, or 0 for the default", lds_width, kCutMaxWidth);
        return cp;
    }
    Trace tr;
    std::vector<char> held;
    cp.plan = build_plan_held(code, L, held, lds_width ? lds_width : kCutMaxWidth, &tr);
    cp.full_width = cp.plan.width;
    if (cp.plan.refusal.code && cp.plan.n_ops == 0) return cp;                  // not a (code, L), or one without a class move: not a matter of width
    if (lds_width == 0) lds_width = default_width(cp.full_width);
    cp.lds_width = lds_width;
    if (cp.full_width - kMaxHeld > lds_width) {
        cp.plan.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "the frontier of code %d at L=%d is %d generators wide: a state vector of width %d needs more than the %d held "
                                                               "generators a cut plan takes (qecmc_class_sweep_tiled keeps a wider state vector in HBM)", code, L, cp.full_width, lds_width, kMaxHeld);
        return cp;
    }
    held.assign((size_t)cp.plan.n_gen, 0);
    while (cp.plan.width > lds_width) {
        const int pick = pick_hold(tr, cp.plan.n_gen);
        if (pick < 0) { cp.plan.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: no generator is live at the peak of code %d at L=%d", code, L); return cp; }
        if (cp.n_held == kMaxHeld) {
            cp.plan.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "the frontier of code %d at L=%d is %d generators wide: %d held generators leave width %d, a state vector of "
                                                                   "width %d needs more than that (qecmc_class_sweep_tiled keeps a wider state vector in HBM)", code, L, cp.full_width, kMaxHeld,
                                            cp.plan.width, lds_width);
            return cp;
        }
        held[(size_t)pick] = 1; ++cp.n_held;
        cp.plan = build_plan_held(code, L, held, lds_width, &tr);
        if (cp.plan.refusal.code && cp.plan.width <= lds_width) return cp;      // (an internal refusal)
    }
    if (cp.plan.refusal.code) return cp;
    held_generator_words(correct::build_table(code, L), held, cp.held, cp.held_words);
    return cp;
}

// How a batch becomes launches: groups of syndromes such that group * ncls * 2^n_held workgroups stay within kCutGridMax, and within kGroupMax
inline uint32_t cut_launch_group(uint64_t N, int ncls, int n_held)
{
    const uint32_t per = (uint32_t)ncls << n_held;
    uint32_t group = kCutGridMax / per;
    if (group < 1u) group = 1u;
    if (group > kGroupMax) group = kGroupMax;
    return N < group ? (N ? (uint32_t)N : 1u) : group;
}

// what every launch of a cut plan's sweep kernel asks of its arguments, whatever the algebra; a launch adds what is its own
inline bool cut_args_ok(uint32_t S, int ncls, int width, int W, int n_ops, int n_held)
{
    return (ncls == 4 || ncls == 16) && cut_fits(width) && W >= 1 && n_ops >= 1 && n_held >= 0 && n_held <= kMaxHeld && S <= cut_launch_group(S, ncls, n_held);
}

// the representative of assignment h: rep times the held generators whose bit is set in h
inline void cut_representative(const CutPlan &cp, const uint32_t *rep, uint32_t h, uint32_t *out)
{
    for (int w = 0; w < cp.plan.W; ++w) {
        uint32_t v = rep[w];
        for (int j = 0; j < cp.n_held; ++j)
            if ((h >> j) & 1u) v ^= cp.held_words[(size_t)j * cp.plan.W + w];
        out[w] = v;
    }
}

// the sum of the partials P[2^n_held] as the reduce kernel forms it, and the scale
inline double cut_reduce(double *P, int n_held, double scale)
{
    for (int j = 0; j < n_held; ++j)
        for (uint32_t k = 0; k < (1u << (n_held - 1 - j)); ++k) {
            const uint32_t h = k << (j + 1);
            P[h] = P[h] + P[h | (1u << j)];
        }
    return P[0] * scale;
}

// The twin.  chains uint8[N][nq], w[4] (I, X, Y, Z) -> Z double[N][ncls]; cls int32[N] (nullable).  The partials of one syndrome are spread over
// `threads` host threads (0: as many as the machine has, 16 at most); every partial and every sum is formed in the same order whatever their number.
inline void sweep_cut_host(const CutPlan &cp, uint64_t N, const uint8_t *chains, const double *w, double *Z, int32_t *cls, unsigned threads = 0)
{
    const Plan &p = cp.plan;
    double wxz[4];
    weights_xz(w, wxz);
    Plan unscaled = p;
    unscaled.scale = 1.0;                                                       // (A[0] * 1.0 is A[0])
    const uint32_t n_h = 1u << cp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = host_threads(threads, n_work, n_work, cp.n_held == 0);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    std::vector<double> P((size_t)n_work);
    for (uint64_t s = 0; s < N; ++s) {
        const int a = class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        host_partials(n_work, threads, p.width, p.W, P.data(), [&](uint32_t i, uint32_t *rep, double *A) {
            cut_representative(cp, &reps[(size_t)(i >> cp.n_held) * p.W], i & (n_h - 1u), rep);
            return sweep_one(unscaled, rep, wxz, A);
        });
        for (int c = 0; c < p.ncls; ++c) Z[s * (uint64_t)p.ncls + c] = cut_reduce(&P[(size_t)c << cp.n_held], cp.n_held, p.scale);
    }
}

}  // namespace sweep

// class_sweep_cut.hip: all pointers are device pointers.  ops uint32[n_ops][4]; held uint32[n_held][W]; reps uint32[S][ncls][W];
// P double[S][ncls][2^n_held]: scratch, every entry written before it is read; z double[S][ncls]: overwritten.
struct SweepCutArgs {
    uint32_t S;
    int ncls, W, width, n_ops, n_held;
    double wxz[4], scale;
};
// The dynamic-LDS limit of one sweep kernel of the family, raised to kCutLdsBudget where a plan of this width needs more than the default window
// (width 14: 128 KiB, one workgroup per CU).  The limit is an attribute of each kernel, so each has a state of its own; it is asked for once per
// device.  hipErrorInvalidValue where the runtime does not grant it -- reported by value, not left behind as the thread's last error -- which the
// entry points report as QECMC_ERR_UNSUPPORTED.
struct LdsOptIn {
    static constexpr int kDevices = 64;
    std::mutex mu;
    signed char state[kDevices] = {};  // 0: not asked, 1: granted, -1: refused
};
hipError_t cut_allow_lds(const void *kernel, LdsOptIn &opt, int width);
hipError_t class_sweep_cut_allow_lds(int width);      // hipSuccess: a state vector of this width can be launched on the current device
hipError_t launch_class_sweep_cut(const SweepCutArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, double *P, double *z, hipStream_t stream);
// k_class_sweep_cut alone: the unscaled partials, left as they are (class_sample.hip picks an assignment from them before anything folds them)
hipError_t launch_class_sweep_cut_partials(const SweepCutArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, double *P, hipStream_t stream);
// k_class_sweep_reduce alone, on the partials of a.S syndromes (n_held, ncls and scale are read): class_sweep_tiled.hip forms its partials itself
hipError_t launch_class_sweep_reduce(const SweepCutArgs &a, double *P, double *z, hipStream_t stream);

}  // namespace qecmc
