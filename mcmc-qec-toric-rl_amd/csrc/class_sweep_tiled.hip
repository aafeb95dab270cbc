// qecmc_class_sweep_tiled: the op stream of class_sweep_tiled.hpp over state vectors double[2^state_bits] in HBM, one launch per segment.
//
// k_class_sweep_tiled: workgroup (blockIdx.x, blockIdx.y) owns live tile blockIdx.x of unit unit_first + blockIdx.y of the pass, a unit being
// ((syndrome * ncls + class) << n_held) + h.  The tile's fixed bits are blockIdx.x spread over the occupied slots outside T, so only live tiles are
// launched and no workgroup exits early.  It gathers the entries live at the segment's first op from the unit's state vector into double[2^tile_width]
// of dynamic LDS -- consecutive lanes read runs of 16 doubles, T holding the low index bits --, runs the segment's ops there with k_class_sweep's
// per-entry code (copies, single multiplies, single adds, one barrier per op) and stores the entries live after its last op.  The ops arrive in the
// tile's coordinates (encode_dev_op); a CLOSE's pairs on fixed slots are decided by the tile's own bits and fold into the qubit's Pauli.  The segment,
// the ops, the representative's words and the held words are kernel arguments or scalar loads under wave-uniform control flow; values leave through
// vector stores.  The first segment gathers nothing and sets A[0] = 1; the last one stores its one live entry as the unit's unscaled partial P[unit].
// Dirty HBM and dirty LDS are allowed: class_sweep_tiled.hpp states the invariant.
//
// The launches of a pass go to one stream in segment order, and k_class_sweep_reduce (class_sweep_cut.hip) after the last pass of a group: stream
// order is the only synchronisation, there are no flags, no atomics and no grid-wide barrier.
#include "class_sweep_tiled.hpp"

namespace qecmc {

__global__ __launch_bounds__(1024) void k_class_sweep_tiled(const SweepTiledArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                            const uint32_t *__restrict__ reps, double *__restrict__ work, double *__restrict__ P)
{
    extern __shared__ double sweep_tile_lds[];                // [2^tile_width]
    const uint32_t tid = threadIdx.x, threads = blockDim.x, unit = a.unit_first + blockIdx.y, hbits = unit & ((1u << a.n_held) - 1u);
    const uint32_t base = sweep::bits_deposit(blockIdx.x, a.fixed_live), entries = 1u << a.tile_width;
    const uint32_t *rep = reps + (size_t)(unit >> a.n_held) * (size_t)a.W;
    double *A = work + ((size_t)blockIdx.y << a.state_bits) + base;
    // local index l <-> offset f = l spread over T; the next one of a lane is `threads` further: an addition that carries across the bits outside T
    const uint32_t f0 = sweep::bits_deposit(tid, a.tile), step = sweep::bits_deposit(threads, a.tile);
    if (a.first) {
        if (tid == 0) sweep_tile_lds[0] = 1.0;
    } else {
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_in)) sweep_tile_lds[l] = A[f];
    }
    __syncthreads();
    for (uint32_t o = a.op_first; o < a.op_first + a.op_count; ++o) {
        const uint32_t w0 = ops[5 * o], mask = ops[5 * o + 1];
        const uint32_t kind = w0 & 15u, slot = (w0 >> 4) & 15u, top = (w0 >> 8) & 31u, bit = 1u << slot;
        if (kind == sweep::kClose) {
            const uint32_t pairs = ops[5 * o + 2], q = ops[5 * o + 3], fixed = ops[5 * o + 4];
            uint32_t word = rep[q >> 4];
            for (uint32_t rest = hbits; rest; rest &= rest - 1u) word ^= held[(uint32_t)(__ffs(rest) - 1) * (uint32_t)a.W + (q >> 4)];
            uint32_t cq = sweep::pauli_to_xz((word >> ((q & 15u) * 2u)) & 3u);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t pr = (fixed >> (8 * j)) & 0xFFu;
                cq ^= (0u - ((base >> (pr & 31u)) & 1u)) & (pr >> 5);
            }
            for (uint32_t f = tid; f < (1u << top); f += threads) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                const double lo = (idx & 1u) ? a.wxz[1] : a.wxz[0], hi = (idx & 1u) ? a.wxz[3] : a.wxz[2];
                sweep_tile_lds[f] = sweep_tile_lds[f] * ((idx & 2u) ? hi : lo);
            }
        } else {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += threads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                if (kind == sweep::kIntro) sweep_tile_lds[f | bit] = sweep_tile_lds[f];
                else sweep_tile_lds[f] = sweep_tile_lds[f] + sweep_tile_lds[f | bit];
            }
        }
        __syncthreads();
    }
    if (a.last) {
        if (tid == 0) P[unit] = sweep_tile_lds[0];
    } else {
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_out)) A[f] = sweep_tile_lds[l];
    }
}

hipError_t launch_class_sweep_tiled(const sweep::TiledPlan &tp, const double *wxz, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                    const uint32_t *reps, double *work, double *P, hipStream_t stream)
{
    if (units == 0) return hipSuccess;
    const sweep::Plan &p = tp.plan;
    if ((p.ncls != 4 && p.ncls != 16) || tp.tile_width < sweep::kTileMinWidth || tp.tile_width > sweep::kTileMaxWidth || tp.state_bits < tp.tile_width ||
        tp.state_bits > sweep::kTiledMaxWidth || p.W < 1 || p.n_ops < 1 || tp.n_held < 0 || tp.n_held > sweep::kMaxHeld || units > sweep::tiled_pass_units(tp.state_bits) ||
        tp.segments.empty())
        return hipErrorInvalidValue;
    SweepTiledArgs a = {};
    a.unit_first = unit_first; a.units = units; a.W = p.W; a.n_held = tp.n_held; a.state_bits = tp.state_bits; a.tile_width = tp.tile_width;
    for (int i = 0; i < 4; ++i) a.wxz[i] = wxz[i];
    for (size_t s = 0; s < tp.segments.size(); ++s) {
        const sweep::Segment &sg = tp.segments[s];
        a.op_first = sg.op_first; a.op_count = sg.op_count; a.tile = sg.tile; a.fixed_live = sg.live & ~sg.tile;
        a.local_in = sweep::bits_extract(sg.live_in, sg.tile); a.local_out = sweep::bits_extract(sg.live_out, sg.tile);
        a.n_tiles = sg.n_tiles; a.first = s == 0; a.last = s + 1 == tp.segments.size();
        if ((int)sweep::popcount32(sg.tile) != tp.tile_width || (sg.tile >> tp.state_bits) != 0u || (sg.live >> tp.state_bits) != 0u ||
            sg.n_tiles != 1u << sweep::popcount32(a.fixed_live) || sg.op_first + sg.op_count > (uint32_t)p.n_ops)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_class_sweep_tiled, dim3(sg.n_tiles, units), dim3(sweep::tiled_threads(tp.tile_width)), sweep::lds_carve(tp.tile_width).bytes, stream, a, dev_ops,
                           held, reps, work, P);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace qecmc
