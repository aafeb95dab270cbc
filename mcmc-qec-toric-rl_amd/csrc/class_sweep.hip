// qecmc_class_sweep: the op stream of class_sweep.hpp over a state vector double[2^width] in LDS; the op loop is class_sweep_ops.hpp's.
//
// Workgroup (blockIdx.x, blockIdx.y) sweeps class blockIdx.x of syndrome blockIdx.y of the group, kThreads lanes.  The four weights and the scale are
// kernel arguments.  The result leaves through one vector store per workgroup.
#include "class_sweep.hpp"

namespace qecmc {

__global__ __launch_bounds__(sweep::kThreads) void k_class_sweep(const SweepArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ reps,
                                                                 double *__restrict__ z)
{
    extern __shared__ double sweep_lds[];                     // [2^width]
    const uint32_t tid = threadIdx.x, pair = blockIdx.y * (uint32_t)a.ncls + blockIdx.x;
    if (tid == 0) sweep_lds[0] = 1.0;
    __syncthreads();
    sweep::op_loop<sweep::NarrowOps, sweep::SumProduct>(sweep_lds, ops, 0u, (uint32_t)a.n_ops, tid, (uint32_t)sweep::kThreads,
                                                        sweep::Rep{reps + (size_t)pair * (size_t)a.W}, sweep::UniformFour<double>{a.wxz});
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
