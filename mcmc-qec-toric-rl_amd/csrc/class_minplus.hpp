// The shortest chain of every class, and how many chains share its length, by the frontier sweep of class_sweep.hpp in another semiring.  The class
// weight Z_c = sum over s of prod_q w(P_q(s)) is a sum-product over the op stream; the same stream in the semiring of (cost, count) pairs under
// (min, +) -- "times" adds costs and keeps the count, "plus" keeps the smaller cost and, on a tie, adds the counts -- gives for every class
//     cost_c  = min over the coset of sum_q cost(P_q),          count_c = the number of chains of the coset that reach it,
// exactly: integer arithmetic, no rounding, no summation order.  At costs (0, 1, 1, 1) this is the minimum-weight decoder for depolarizing noise
// over Pauli chains (a Y costs 1), and count_c * base^cost_c is the exact value of what the shortest-chain estimators converge to.
//
// THE PLANS are the cut plans of class_sweep_cut.hpp, unchanged: build_cut_plan(code, L, lds_width), class_representatives, cut_representative,
// cut_launch_group and cut_threads.  A cut plan with nothing held is the plain plan, so one path serves both.  What the cut plan refuses is refused
// here with its message prefixed "qecmc_class_minplus:", before a device is looked for.
//
// THE ENTRY is one uint64_t per state-vector entry, cost in bits 63..48 and count in bits 47..0 -- the footprint of the double it replaces, so
// lds_carve, the widths, the grids and the 128 KiB opt-in carry over.  A[0] = (0, 1); INTRO copies; CLOSE adds cost_xz[idx] << 48, idx formed as in
// sweep_one; FORGET is mp_combine.  Counts saturate at kSat = 2^48 - 1, stickily; both operations are associative and commutative, so the partials
// over the held assignments may be combined in any order and the kernels (class_minplus.hip) equal the twin exactly, whatever their order.
//
// THE RESULT per (syndrome, class): cost uint32; count uint64 = the entry's count >> (n_gen - rank) -- every group element is met 2^(n_gen - rank)
// times with the same cost, so the shift is exact.  An entry whose count reached kSat is reported as count = 0: a true count is never 0.
//
// Costs: four integers for I, X, Y, Z, 0 .. 255 each; zero is allowed anywhere and so is a non-zero cost of I.  A cost above 255 is refused by name
// (QECMC_ERR_INVALID).  The cost of a chain is at most n_qubits * 255 < 2^16 at every accepted shape (check_cost_range), so the cost field never
// carries into nothing and never wraps.
#pragma once
#include "class_sweep_cut.hpp"

namespace qecmc {
namespace minplus {

constexpr int kCountBits = 48;
constexpr uint64_t kSat = (1ull << kCountBits) - 1ull;      // a count that reached it stays there
constexpr uint32_t kMaxCost = 255;
static_assert(sizeof(uint64_t) == sizeof(double), "the entry takes the place of the sweep's double: lds_carve is shared");
static_assert(11 * 11 * kMaxCost < (1u << 16) && 2 * 7 * 7 * kMaxCost < (1u << 16) && 2 * 5 * 5 * kMaxCost < (1u << 16),
              "the dearest chain of the widest accepted shapes (rotated L = 11, planar L = 7, toric L = 5) fits the 16 bits of the cost");

// a, b <= kSat: min(a + b, kSat)
__host__ __device__ inline uint64_t mp_sat_add(uint64_t a, uint64_t b)
{
    const uint64_t s = a + b;
    return s > kSat ? kSat : s;
}

// the entry with the smaller cost; on equal cost, that cost with the saturating sum of the counts
__host__ __device__ inline uint64_t mp_combine(uint64_t a, uint64_t b)
{
    const uint64_t ca = a >> kCountBits, cb = b >> kCountBits;
    if (ca != cb) return ca < cb ? a : b;
    return (ca << kCountBits) | mp_sat_add(a & kSat, b & kSat);
}

inline Refusal check_costs(const uint32_t *cost)
{
    for (int i = 0; i < 4; ++i)
        if (cost[i] > kMaxCost)
            return refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus: cost[%d]=%u: the costs of I, X, Y and Z are integers 0 .. %u", i, cost[i], kMaxCost);
    return {};
}

// the host check behind the static_assert above, at the plan's own figures
inline Refusal check_cost_range(const sweep::Plan &p)
{
    if ((uint64_t)p.n_qubits * kMaxCost >= (1ull << 16))
        return refuse_params(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus: %d qubits at a cost of up to %u each leave the 16 bits of an entry's cost", p.n_qubits, kMaxCost);
    return {};
}

// build_cut_plan with the cut plan's refusal prefixed, and the cost range checked
inline sweep::CutPlan build_minplus_plan(int code, int L, int lds_width)
{
    sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    if (cp.plan.refusal.code) cp.plan.refusal.msg = "qecmc_class_minplus: " + cp.plan.refusal.msg;
    else cp.plan.refusal = check_cost_range(cp.plan);
    return cp;
}

// the cost table in (x, z) order: I, X, Z, Y
inline void costs_xz(const uint32_t *cost, uint32_t *cxz) { cxz[0] = cost[0]; cxz[1] = cost[1]; cxz[2] = cost[3]; cxz[3] = cost[2]; }

// one representative (packed words) through the op stream: the twin of one workgroup of k_class_minplus.  A: 2^width entries of scratch, dirty allowed.
// -> the packed partial
inline uint64_t minplus_one(const sweep::Plan &p, const uint32_t *rep, const uint32_t *cxz, uint64_t *A)
{
    A[0] = 1ull;                                                                // (0, 1)
    sweep::host_ops(p.ops.data(), p.n_ops, rep, A, [&](uint64_t a, uint32_t, uint32_t idx) { return a + ((uint64_t)cxz[idx] << kCountBits); }, mp_combine,
                    sweep::NoDecisions{});
    return A[0];
}

// a packed entry as the result: the cost, and the count shifted by n_gen - rank -- 0 where it saturated
__host__ __device__ inline void mp_unpack(uint64_t e, int shift, uint32_t *cost, uint64_t *count)
{
    const uint64_t n = e & kSat;
    *cost = (uint32_t)(e >> kCountBits);
    *count = n == kSat ? 0ull : n >> shift;
}

// The twin.  chains uint8[N][nq], cost4[4] (I, X, Y, Z) -> cost_out uint32[N][ncls], count_out uint64[N][ncls]; cls int32[N] (nullable).  Threaded
// as sweep_cut_host: the partials of one syndrome are spread over `threads` host threads (0: as many as the machine has, 16 at most).
inline void minplus_cut_host(const sweep::CutPlan &cp, uint64_t N, const uint8_t *chains, const uint32_t *cost4, uint32_t *cost_out, uint64_t *count_out, int32_t *cls,
                             unsigned threads = 0)
{
    const sweep::Plan &p = cp.plan;
    uint32_t cxz[4];
    costs_xz(cost4, cxz);
    const uint32_t n_h = 1u << cp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = sweep::host_threads(threads, n_work, n_work, cp.n_held == 0);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    std::vector<uint64_t> P((size_t)n_work);
    for (uint64_t s = 0; s < N; ++s) {
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        sweep::host_partials(n_work, threads, p.width, p.W, P.data(), [&](uint32_t i, uint32_t *rep, uint64_t *A) {
            sweep::cut_representative(cp, &reps[(size_t)(i >> cp.n_held) * p.W], i & (n_h - 1u), rep);
            return minplus_one(p, rep, cxz, A);
        });
        for (int c = 0; c < p.ncls; ++c) {
            uint64_t e = P[(size_t)c << cp.n_held];
            for (uint32_t h = 1; h < n_h; ++h) e = mp_combine(e, P[((size_t)c << cp.n_held) + h]);
            mp_unpack(e, p.n_gen - p.rank, &cost_out[s * (uint64_t)p.ncls + c], &count_out[s * (uint64_t)p.ncls + c]);
        }
    }
}

#ifdef __HIPCC__
// the device algebra (class_sweep_ops.hpp): a CLOSE adds the cost to the upper 16 bits, a FORGET is mp_combine
struct MinPlus {
    static __device__ __forceinline__ uint64_t close(uint64_t a, uint32_t cost) { return a + ((uint64_t)cost << kCountBits); }
    static __device__ __forceinline__ uint64_t forget(uint64_t a, uint64_t b) { return mp_combine(a, b); }
};
#endif

}  // namespace minplus

// class_minplus.hip: all pointers are device pointers.  ops uint32[n_ops][4]; held uint32[n_held][W]; reps uint32[S][ncls][W];
// P uint64[S][ncls][2^n_held]: scratch, every entry written before it is read; cost_out uint32[S][ncls], count_out uint64[S][ncls]: overwritten.
struct MinplusArgs {
    uint32_t S;
    int ncls, W, width, n_ops, n_held, shift;          // shift: n_gen - rank
    uint32_t cxz[4];                                   // the costs in (x, z) order
};
hipError_t class_minplus_allow_lds(int width);         // hipSuccess: a state vector of this width can be launched on the current device
hipError_t launch_class_minplus(const MinplusArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, uint64_t *P, uint32_t *cost_out, uint64_t *count_out,
                                hipStream_t stream);
// its two launches, one each: class_minplus_trace.hip reads the partials between them (the reduce folds them in place)
hipError_t launch_class_minplus_sweep(const MinplusArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, uint64_t *P, hipStream_t stream);
hipError_t launch_class_minplus_reduce(const MinplusArgs &a, uint64_t *P, uint32_t *cost_out, uint64_t *count_out, hipStream_t stream);

}  // namespace qecmc
