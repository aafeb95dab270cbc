// qecmc_class_sweep_tiled: the op stream of class_sweep_tiled.hpp over state vectors double[2^state_bits] in HBM, one launch per segment.
//
// k_class_sweep_tiled: workgroup (blockIdx.x, blockIdx.y) owns live tile blockIdx.x of unit unit_first + blockIdx.y of the pass, a unit being
// ((syndrome * ncls + class) << n_held) + h.  The tile's fixed bits are blockIdx.x spread over the occupied slots outside T, so only live tiles are
// launched and no workgroup exits early.  It gathers the entries live at the segment's first op from the unit's state vector into double[2^tile_width]
// of dynamic LDS -- consecutive lanes read runs of 16 doubles, T holding the low index bits --, runs the segment's ops there with the op loop of
// class_sweep_ops.hpp and stores the entries live after its last op (sweep::tile_sweep, which k_class_sweep_tiled_site shares).  The ops arrive in
// the tile's coordinates (encode_dev_op); a CLOSE's pairs on fixed slots are decided by the tile's own bits and fold into the qubit's Pauli.  The
// segment, the ops, the representative's words and the held words are kernel arguments or scalar loads under wave-uniform control flow; values leave
// through vector stores.  The first segment gathers nothing and sets A[0] = 1; the last one stores its one live entry as the unit's unscaled partial
// P[unit].  Dirty HBM and dirty LDS are allowed: class_sweep_tiled.hpp states the invariant.
//
// The launches of a pass go to one stream in segment order, and k_class_sweep_reduce (class_sweep_cut.hip) after the last pass of a group: stream
// order is the only synchronisation, there are no flags, no atomics and no grid-wide barrier.
#include "class_sweep_tiled.hpp"

namespace qecmc {

__global__ __launch_bounds__(1024) void k_class_sweep_tiled(const SweepTiledArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                            const uint32_t *__restrict__ reps, double *__restrict__ work, double *__restrict__ P)
{
    extern __shared__ double sweep_tile_lds[];                // [2^tile_width]
    sweep::tile_sweep<sweep::SumProduct>(sweep_tile_lds, a, ops, held, reps, work, P, sweep::UniformFour<double>{a.wxz});
}

hipError_t launch_class_sweep_tiled(const sweep::TiledPlan &tp, const double *wxz, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                    const uint32_t *reps, double *work, double *P, hipStream_t stream)
{
    if (units == 0) return hipSuccess;
    SweepTiledArgs a = {};
    for (int i = 0; i < 4; ++i) a.wxz[i] = wxz[i];
    return sweep::tiled_segments(tp, unit_first, units, a, [&](const SweepTiledArgs &seg, const sweep::Segment &sg) {
        hipLaunchKernelGGL(k_class_sweep_tiled, dim3(sg.n_tiles, units), dim3(sweep::tiled_threads(tp.tile_width)), sweep::lds_carve(tp.tile_width).bytes, stream, seg,
                           dev_ops, held, reps, work, P);
    });
}

}  // namespace qecmc
