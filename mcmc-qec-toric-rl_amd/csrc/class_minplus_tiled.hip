// qecmc_class_minplus_tiled, qecmc_class_minplus_tiled_site: the (min, +, count) sweep of class_minplus.hpp over state vectors uint64_t[2^state_bits] in
// HBM, one launch per segment of the tiled plan (class_minplus_tiled.hpp).
//
// Each kernel has its sum-product sibling's grid, block, LDS and body -- k_class_sweep_tiled (class_sweep_tiled.hip), k_class_sweep_tiled_site
// (class_sweep_site.hip): workgroup (blockIdx.x, blockIdx.y) owns live tile blockIdx.x of unit unit_first + blockIdx.y of the pass, gathers the entries
// live at the segment's first op into uint64_t[2^tile_width] of dynamic LDS, runs the segment's ops there and stores the entries live after its last op
// (sweep::tile_sweep).  What is theirs is the entry and its algebra: a packed (cost, count) word where the siblings keep a double, minplus::MinPlus in
// the op loop of class_sweep_ops.hpp -- CLOSE adds the cost of the qubit's Pauli to the upper 16 bits, FORGET is mp_combine.  The first segment gathers
// nothing and sets A[0] = (0, 1); the last one stores its one live entry as the unit's packed partial P[unit].  Dirty HBM and dirty LDS are allowed:
// class_sweep_tiled.hpp states the invariant, and the workspace is shared with the sum-product sweeps.
//
// k_class_minplus_tiled takes the four costs as kernel arguments.  k_class_minplus_tiled_site reads the cost word cw[(per_syndrome ? syndrome : 0) * nq
// + q] of a CLOSE's qubit, the syndrome from the block index alone ((unit >> n_held) / ncls) and q from the plan: a wave-uniform address, one scalar
// load per CLOSE, as class_minplus_site.hip does it.  Values leave through vector stores.  No atomics, no flags, no scratch, no static LDS.
//
// The launches of a pass go to one stream in segment order, and k_class_minplus_reduce (class_minplus.hip) after the last pass of a group: stream
// order is the only synchronisation.
#include "class_minplus_tiled.hpp"

namespace qecmc {

__global__ __launch_bounds__(1024) void k_class_minplus_tiled(const MinplusTiledArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                              const uint32_t *__restrict__ reps, uint64_t *__restrict__ work, uint64_t *__restrict__ P)
{
    extern __shared__ uint64_t minplus_tile_lds[];            // [2^tile_width]
    sweep::tile_sweep<minplus::MinPlus>(minplus_tile_lds, a, ops, held, reps, work, P, sweep::UniformFour<uint32_t>{a.cxz});
}

__global__ __launch_bounds__(1024) void k_class_minplus_tiled_site(const MinplusTiledSiteArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                   const uint32_t *__restrict__ reps, const uint32_t *__restrict__ cw, uint64_t *__restrict__ work,
                                                                   uint64_t *__restrict__ P)
{
    extern __shared__ uint64_t minplus_tile_site_lds[];       // [2^tile_width]
    const uint32_t unit = a.unit_first + blockIdx.y;
    const uint32_t *row = cw + (size_t)(a.per_syndrome ? (unit >> a.n_held) / (uint32_t)a.ncls : 0u) * (size_t)a.nq;
    sweep::tile_sweep<minplus::MinPlus>(minplus_tile_site_lds, a, ops, held, reps, work, P, minplus::SiteCosts{row});
}

hipError_t launch_class_minplus_tiled(const sweep::TiledPlan &tp, const uint32_t *cxz, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                      const uint32_t *reps, uint64_t *work, uint64_t *P, hipStream_t stream)
{
    if (units == 0) return hipSuccess;
    MinplusTiledArgs a = {};
    for (int i = 0; i < 4; ++i) a.cxz[i] = cxz[i];
    return sweep::tiled_segments(tp, unit_first, units, a, [&](const MinplusTiledArgs &seg, const sweep::Segment &sg) {
        hipLaunchKernelGGL(k_class_minplus_tiled, dim3(sg.n_tiles, units), dim3(sweep::tiled_threads(tp.tile_width)), sweep::lds_carve(tp.tile_width).bytes, stream, seg,
                           dev_ops, held, reps, work, P);
    });
}

hipError_t launch_class_minplus_tiled_site(const sweep::TiledPlan &tp, int per_syndrome, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                           const uint32_t *reps, const uint32_t *cw, uint64_t *work, uint64_t *P, hipStream_t stream)
{
    if (units == 0) return hipSuccess;
    if (!cw || tp.plan.nq < 1 || (per_syndrome != 0 && per_syndrome != 1)) return hipErrorInvalidValue;
    MinplusTiledSiteArgs a = {};
    a.ncls = tp.plan.ncls; a.nq = tp.plan.nq; a.per_syndrome = per_syndrome;
    return sweep::tiled_segments(tp, unit_first, units, a, [&](const MinplusTiledSiteArgs &seg, const sweep::Segment &sg) {
        hipLaunchKernelGGL(k_class_minplus_tiled_site, dim3(sg.n_tiles, units), dim3(sweep::tiled_threads(tp.tile_width)), sweep::lds_carve(tp.tile_width).bytes, stream, seg,
                           dev_ops, held, reps, cw, work, P);
    });
}

}  // namespace qecmc
