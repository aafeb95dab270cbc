// qecmc_class_sweep: the op stream of class_sweep.hpp over a state vector double[2^width] in LDS, updated in place.
//
// Workgroup (blockIdx.x, blockIdx.y) sweeps class blockIdx.x of syndrome blockIdx.y of the group.  The plan is the same for every workgroup and is
// addressed by the loop counter alone, the representative's packed words by the block index and the op's qubit: scalar loads, wave-uniform control
// flow; the four weights and the scale are kernel arguments.  An op walks the indices below its `top` -- the ranges above the highest occupied slot
// are skipped -- and leaves out an index with a bit outside its mask: only live entries are read, and every live entry was written by the INTRO that
// made it live, so dirty LDS does not matter (A[0] = 1 is the one word the kernel sets up).  One barrier after every op.  INTRO and FORGET walk the
// half index h with a zero inserted at the slot: consecutive lanes touch consecutive 8-byte entries in runs of 2^slot, so slots below 4 read two
// 256-byte bank rows per 32-lane group (2-way) and the others one; CLOSE is unit stride.  Every entry sees exactly the operation sequence of
// sweep_one(): copies, single multiplies, single adds.  The result leaves through one vector store per workgroup.  Nothing here grows with N.
#include "class_sweep.hpp"

namespace qecmc {

__global__ __launch_bounds__(sweep::kThreads) void k_class_sweep(const SweepArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ reps,
                                                                 double *__restrict__ z)
{
    extern __shared__ double sweep_lds[];                     // [2^width]
    const uint32_t tid = threadIdx.x, pair = blockIdx.y * (uint32_t)a.ncls + blockIdx.x;
    const uint32_t *rep = reps + (size_t)pair * (size_t)a.W;
    if (tid == 0) sweep_lds[0] = 1.0;
    __syncthreads();
    for (int o = 0; o < a.n_ops; ++o) {
        const uint32_t w0 = ops[4 * o], mask = ops[4 * o + 1];
        const uint32_t kind = w0 & 15u, slot = (w0 >> 4) & 15u, top = (w0 >> 12) & 31u, bit = 1u << slot;
        if (kind == sweep::kClose) {
            const uint32_t pairs = ops[4 * o + 2], q = ops[4 * o + 3];
            const uint32_t cq = sweep::pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
            for (uint32_t f = tid; f < (1u << top); f += sweep::kThreads) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                const double lo = (idx & 1u) ? a.wxz[1] : a.wxz[0], hi = (idx & 1u) ? a.wxz[3] : a.wxz[2];
                sweep_lds[f] = sweep_lds[f] * ((idx & 2u) ? hi : lo);
            }
        } else {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += sweep::kThreads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                if (kind == sweep::kIntro) sweep_lds[f | bit] = sweep_lds[f];
                else sweep_lds[f] = sweep_lds[f] + sweep_lds[f | bit];
            }
        }
        __syncthreads();
    }
    if (tid == 0) z[pair] = sweep_lds[0] * a.scale;
}

hipError_t launch_class_sweep(const SweepArgs &a, const uint32_t *ops, const uint32_t *reps, double *z, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if ((a.ncls != 4 && a.ncls != 16) || a.width < 1 || a.width > sweep::kMaxWidth || carve.bytes == 0 || carve.bytes > sweep::kLdsBudget || a.W < 1 ||
        a.n_ops < 1 || a.S > sweep::kGroupMax)
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)a.ncls, a.S), block(sweep::kThreads);
    hipLaunchKernelGGL(k_class_sweep, grid, block, carve.bytes, stream, a, ops, reps, z);
    return hipGetLastError();
}

}  // namespace qecmc
