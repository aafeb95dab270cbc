// qecmc_class_sweep_cut: the cut-set sweep of class_sweep_cut.hpp; the op loop is class_sweep_ops.hpp's.
//
// k_class_sweep_cut: workgroup blockIdx.x = ((syndrome * ncls + class) << n_held) + h sweeps one representative under one assignment h of the held
// generators, cut_threads(width) lanes.  The representative is formed where an op needs it: the packed word of the op's qubit, XOR the same word of
// every held generator whose bit is set in h -- h comes from the block index, so these are scalar loads under wave-uniform control flow, as the
// plan's are.  The four weights are kernel arguments.  The unscaled partial leaves through one vector store, P[blockIdx.x].
//
// k_class_sweep_reduce: workgroup blockIdx.x = syndrome * ncls + class sums its 2^n_held partials in place as a FORGET on the held bits, in ascending
// order of the bit -- cut_reduce()'s sequence, one barrier per bit -- and writes z = P[0] * scale.  It is launched on the same stream after the sweep
// kernel: stream order is the only synchronisation, there are no flags and no atomics.
#include "class_sweep_cut.hpp"

namespace qecmc {

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_sweep_cut(const SweepCutArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                     const uint32_t *__restrict__ reps, double *__restrict__ P)
{
    extern __shared__ double sweep_cut_lds[];                 // [2^width]
    const uint32_t tid = threadIdx.x, pair = blockIdx.x >> a.n_held, hbits = blockIdx.x & ((1u << a.n_held) - 1u);
    if (tid == 0) sweep_cut_lds[0] = 1.0;
    __syncthreads();
    sweep::op_loop<sweep::NarrowOps, sweep::SumProduct>(sweep_cut_lds, ops, 0u, (uint32_t)a.n_ops, tid, blockDim.x,
                                                        sweep::HeldRep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W},
                                                        sweep::UniformFour<double>{a.wxz});
    if (tid == 0) P[blockIdx.x] = sweep_cut_lds[0];
}

__global__ __launch_bounds__(sweep::kThreads) void k_class_sweep_reduce(const SweepCutArgs a, double *P, double *z)
{
    double *mine = P + ((size_t)blockIdx.x << a.n_held);
    for (int j = 0; j < a.n_held; ++j) {
        for (uint32_t k = threadIdx.x; k < (1u << (a.n_held - 1 - j)); k += sweep::kThreads) {
            const uint32_t h = k << (j + 1);
            mine[h] = mine[h] + mine[h | (1u << j)];
        }
        __syncthreads();                                      // (the next bit reads what other lanes of this workgroup wrote)
    }
    if (threadIdx.x == 0) z[blockIdx.x] = mine[0] * a.scale;
}

hipError_t cut_allow_lds(const void *kernel, LdsOptIn &opt, int width)
{
    if (!sweep::cut_fits(width)) return hipErrorInvalidValue;
    if (sweep::lds_carve(width).bytes <= sweep::kLdsBudget) return hipSuccess;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= LdsOptIn::kDevices) return hipErrorInvalidValue;
    std::lock_guard<std::mutex> g(opt.mu);
    if (opt.state[dev] == 0) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sweep::kCutLdsBudget);
        if (e != hipSuccess) (void)hipGetLastError();         // (the refusal is reported by value; it is not left behind as the thread's last error)
        opt.state[dev] = e == hipSuccess ? 1 : -1;
    }
    return opt.state[dev] == 1 ? hipSuccess : hipErrorInvalidValue;
}

hipError_t class_sweep_cut_allow_lds(int width)
{
    static LdsOptIn opt;
    return cut_allow_lds(reinterpret_cast<const void *>(k_class_sweep_cut), opt, width);
}

hipError_t launch_class_sweep_cut_partials(const SweepCutArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, double *P, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if (!sweep::cut_args_ok(a.S, a.ncls, a.width, a.W, a.n_ops, a.n_held)) return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_sweep_cut_allow_lds(a.width)) return e;
    const uint32_t pairs = a.S * (uint32_t)a.ncls;
    hipLaunchKernelGGL(k_class_sweep_cut, dim3(pairs << a.n_held), dim3(sweep::cut_threads(a.width)), carve.bytes, stream, a, ops, held, reps, P);
    return hipGetLastError();
}

hipError_t launch_class_sweep_cut(const SweepCutArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, double *P, double *z, hipStream_t stream)
{
    if (hipError_t e = launch_class_sweep_cut_partials(a, ops, held, reps, P, stream)) return e;
    return launch_class_sweep_reduce(a, P, z, stream);
}

hipError_t launch_class_sweep_reduce(const SweepCutArgs &a, double *P, double *z, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if ((a.ncls != 4 && a.ncls != 16) || a.n_held < 0 || a.n_held > sweep::kMaxHeld || a.S > sweep::cut_launch_group(a.S, a.ncls, a.n_held)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_class_sweep_reduce, dim3(a.S * (uint32_t)a.ncls), dim3(sweep::kThreads), 0, stream, a, P, z);
    return hipGetLastError();
}

}  // namespace qecmc
