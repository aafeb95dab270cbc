// The (min, +, count) sweep of class_minplus.hpp on the state vector tiled over HBM of class_sweep_tiled.hpp: the least cost of every class and the
// number of chains that reach it at the shapes only the tiled route takes -- xzzx / rotated L = 13 .. 21, planar L = 8 .. 12, the toric code at L = 7.
//
// THE PLAN is build_tiled_plan(code, L, hbm_width, tile_width), unchanged: the wide op stream, the holds, the segment table and the device ops; the
// launch order (tiled_segments), the units of a pass (tiled_pass_units), the threads of a workgroup (tiled_threads), the 1 GiB workspace, the pass and
// group splitting and TileRep with its fixed-slot pairs are the tiled sweep's.  What it refuses is refused here with its code and its message
// prefixed "qecmc_class_minplus_tiled:" / "qecmc_class_minplus_tiled_site:", before a device is looked for.
//
// THE ENTRY is class_minplus.hpp's uint64_t -- cost in bits 63..48, count in bits 47..0 -- in the place of the sweep's double: a state vector, a
// tile and a partial take the bytes they take there.  A[0] = (0, 1); INTRO and the moves between HBM and LDS copy; CLOSE adds the cost of the
// qubit's Pauli to the upper 16 bits; FORGET is mp_combine.  The partials P[S][ncls][2^n_held] over the held assignments fold with mp_combine in
// k_class_minplus_reduce (class_minplus.hip), and mp_unpack gives cost uint32 and count uint64 >> (n_gen - rank), 0 where saturated.  Integer
// throughout, both operations associative and commutative: the kernels (class_minplus_tiled.hip) equal the twin exactly for every tile_width, and
// where the holds are the cut plan's (hbm_width = its lds_width) the result is qecmc_class_minplus's.
//
// DIRTY MEMORY.  The workspace is the tiled sweep's own block, never cleared, and holds that sweep's doubles between calls; LDS is not cleared
// either.  The invariant of class_sweep_tiled.hpp holds whatever the entry: a live entry is written by the INTRO that made it live before anything
// reads it, a gather reads what the segment before stored.
//
// THE COST RANGE.  The 16 bits of the cost do not cover 255 per qubit here (rotated L = 21 has 441 qubits, planar L = 12 has 265), so the range is
// checked against the call's own costs, before a device is looked for (QECMC_ERR_UNSUPPORTED, by name): n_qubits * max(cost) < 2^16 for the four
// costs; for a site table, the sum over the qubits some CLOSE names of the row's largest cost at the qubit < 2^16 in every row, the first row that
// passes it named.  No chain then costs 2^16 or more, so the cost field neither wraps nor carries into nothing.
#pragma once
#include "class_minplus_site.hpp"

namespace qecmc {
namespace minplus {

constexpr uint64_t kCostLimit = 1ull << (64 - kCountBits);      // a chain's cost stays below it

// build_tiled_plan with its refusal under the entry point's name ("qecmc_class_minplus_tiled" / "qecmc_class_minplus_tiled_site")
inline sweep::TiledPlan build_minplus_tiled_plan(int code, int L, int hbm_width, int tile_width, const char *entry)
{
    sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (tp.plan.refusal.code) tp.plan.refusal.msg = std::string(entry) + ": " + tp.plan.refusal.msg;
    return tp;
}

inline Refusal check_tiled_costs(const uint32_t *cost) { return site_prefix(check_costs(cost), "qecmc_class_minplus:", "qecmc_class_minplus_tiled:"); }

// the four costs against the 16 bits of an entry's cost, at the plan's own qubit count
inline Refusal check_tiled_cost_range(const sweep::Plan &p, const uint32_t *cost)
{
    uint32_t top = 0;
    for (int i = 0; i < 4; ++i) top = cost[i] > top ? cost[i] : top;
    if ((uint64_t)p.n_qubits * top >= kCostLimit)
        return refuse_params(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_tiled: %d qubits at a cost of up to %u each leave the 16 bits of an entry's cost (%d * %u >= %llu)",
                             p.n_qubits, top, p.n_qubits, top, (unsigned long long)kCostLimit);
    return {};
}

// every row of a site table: the dearest chain it prices, over the qubits `named` marks (sweep::closed_qubits)
inline Refusal check_tiled_cost_rows_range(const uint8_t *cq, uint64_t rows, int nq, const std::vector<char> &named)
{
    for (uint64_t r = 0; r < rows; ++r) {
        uint64_t sum = 0;
        for (int q = 0; q < nq; ++q) {
            if (!named[(size_t)q]) continue;
            const uint8_t *c = cq + (r * (uint64_t)nq + (uint64_t)q) * 4u;
            uint32_t top = c[0];
            for (int i = 1; i < 4; ++i) top = c[i] > top ? c[i] : top;
            sum += top;
        }
        if (sum >= kCostLimit)
            return refuse_params(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_tiled_site: cq row %llu: the largest costs of its qubits sum to %llu, which leaves the 16 bits of an "
                                                        "entry's cost (< %llu)", (unsigned long long)r, (unsigned long long)sum, (unsigned long long)kCostLimit);
    }
    return {};
}

// one representative through the wide stream: minplus_one() entry for entry, walking the live indices only.  A: 2^width entries, dirty allowed
inline uint64_t minplus_one_wide(const sweep::TiledPlan &tp, const uint32_t *rep, const uint32_t *cxz, uint64_t *A)
{
    A[0] = 1ull;                                                                // (0, 1)
    sweep::host_ops_wide(tp.ops.data(), tp.plan.n_ops, rep, A, [&](uint64_t a, uint32_t, uint32_t idx) { return a + ((uint64_t)cxz[idx] << kCountBits); }, mp_combine);
    return A[0];
}

// ... with the cost word of the CLOSE's qubit: cw uint32[nq]
inline uint64_t minplus_one_wide_site(const sweep::TiledPlan &tp, const uint32_t *rep, const uint32_t *cw, uint64_t *A)
{
    A[0] = 1ull;
    sweep::host_ops_wide(tp.ops.data(), tp.plan.n_ops, rep, A, [&](uint64_t a, uint32_t q, uint32_t idx) { return a + ((uint64_t)site_cost(cw[q], idx) << kCountBits); },
                         mp_combine);
    return A[0];
}

// the partials of one syndrome, spread over host threads as sweep_tiled_host spreads them, then folded per class: one(rep, A) -> the packed partial
template <class One>
inline void tiled_partials_fold(const sweep::TiledPlan &tp, const uint32_t *reps, unsigned threads, uint64_t *P, uint32_t *cost_out, uint64_t *count_out, One one)
{
    const sweep::Plan &p = tp.plan;
    const uint32_t n_h = 1u << tp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = sweep::host_threads(threads, n_work, sweep::tiled_pass_units(p.width), p.width < 12);
    sweep::host_partials(n_work, threads, p.width, p.W, P, [&](uint32_t i, uint32_t *rep, uint64_t *A) {
        sweep::tiled_representative(tp, &reps[(size_t)(i >> tp.n_held) * p.W], i & (n_h - 1u), rep);
        return one(rep, A);
    });
    for (int c = 0; c < p.ncls; ++c) {
        uint64_t e = P[(size_t)c << tp.n_held];
        for (uint32_t h = 1; h < n_h; ++h) e = mp_combine(e, P[((size_t)c << tp.n_held) + h]);
        mp_unpack(e, p.n_gen - p.rank, &cost_out[c], &count_out[c]);
    }
}

// The twin of qecmc_class_minplus_tiled.  chains uint8[N][nq], cost4[4] (I, X, Y, Z) -> cost_out uint32[N][ncls], count_out uint64[N][ncls];
// cls int32[N] (nullable).  threads: 0 is as many as the machine has, 16 at most, and no more than keep their state vectors within the workspace.
inline void minplus_tiled_host(const sweep::TiledPlan &tp, uint64_t N, const uint8_t *chains, const uint32_t *cost4, uint32_t *cost_out, uint64_t *count_out, int32_t *cls,
                               unsigned threads = 0)
{
    const sweep::Plan &p = tp.plan;
    uint32_t cxz[4];
    costs_xz(cost4, cxz);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    std::vector<uint64_t> P((size_t)p.ncls << tp.n_held);
    for (uint64_t s = 0; s < N; ++s) {
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        tiled_partials_fold(tp, reps.data(), threads, P.data(), cost_out + s * (uint64_t)p.ncls, count_out + s * (uint64_t)p.ncls,
                            [&](const uint32_t *rep, uint64_t *A) { return minplus_one_wide(tp, rep, cxz, A); });
    }
}

// The twin of qecmc_class_minplus_tiled_site.  cq uint8[cq_rows][nq][4] (I, X, Y, Z), cq_rows 1 or N
inline void minplus_tiled_site_host(const sweep::TiledPlan &tp, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, uint32_t *cost_out, uint64_t *count_out,
                                    int32_t *cls, unsigned threads = 0)
{
    const sweep::Plan &p = tp.plan;
    const size_t row = (size_t)p.nq * 4u;
    std::vector<uint32_t> cw((size_t)p.nq), reps((size_t)p.ncls * p.W);
    std::vector<uint64_t> P((size_t)p.ncls << tp.n_held);
    for (uint64_t s = 0; s < N; ++s) {
        if (s == 0 || cq_rows != 1) site_cost_words(cq + (cq_rows == 1 ? 0u : s) * row, 1, p.nq, cw.data());
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        tiled_partials_fold(tp, reps.data(), threads, P.data(), cost_out + s * (uint64_t)p.ncls, count_out + s * (uint64_t)p.ncls,
                            [&](const uint32_t *rep, uint64_t *A) { return minplus_one_wide_site(tp, rep, cw.data(), A); });
    }
}

}  // namespace minplus

// class_minplus_tiled.hip: all pointers are device pointers.  dev_ops, held, reps as class_sweep_tiled.hip takes them; work uint64[units][2^state_bits]:
// the state vectors of one pass, dirty; P uint64[S][ncls][2^n_held]: every entry written before launch_class_minplus_reduce reads it;
// cw uint32[per_syndrome ? S : 1][nq]: a word per qubit in (x, z) byte order, S counting the syndromes of the launch group.
struct MinplusTiledArgs {
    uint32_t unit_first, units;        // as SweepTiledArgs, the four weights being the four costs in (x, z) order
    int W, n_held, state_bits, tile_width;
    uint32_t op_first, op_count, tile, fixed_live, local_in, local_out, n_tiles, first, last;
    uint32_t cxz[4];
};
struct MinplusTiledSiteArgs {
    uint32_t unit_first, units;        // as SweepTiledSiteArgs
    int W, n_held, state_bits, tile_width;
    uint32_t op_first, op_count, tile, fixed_live, local_in, local_out, n_tiles, first, last;
    int ncls, nq, per_syndrome;
};
hipError_t launch_class_minplus_tiled(const sweep::TiledPlan &tp, const uint32_t *cxz, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                      const uint32_t *reps, uint64_t *work, uint64_t *P, hipStream_t stream);
hipError_t launch_class_minplus_tiled_site(const sweep::TiledPlan &tp, int per_syndrome, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                           const uint32_t *reps, const uint32_t *cw, uint64_t *work, uint64_t *P, hipStream_t stream);

}  // namespace qecmc
