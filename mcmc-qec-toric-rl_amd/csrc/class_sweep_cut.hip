// qecmc_class_sweep_cut: the cut-set sweep of class_sweep_cut.hpp.
//
// k_class_sweep_cut: workgroup blockIdx.x = ((syndrome * ncls + class) << n_held) + h sweeps one representative under one assignment h of the held
// generators.  The representative is formed where an op needs it: the packed word of the op's qubit, XOR the same word of every held generator whose
// bit is set in h -- h comes from the block index, so these are scalar loads under wave-uniform control flow, as the plan's are.  The op loop is
// k_class_sweep's (class_sweep.hip), entry for entry: copies, single multiplies, single adds on double[2^width] in dynamic LDS, one barrier per op,
// dirty LDS allowed.  The unscaled partial leaves through one vector store, P[blockIdx.x].
//
// k_class_sweep_reduce: workgroup blockIdx.x = syndrome * ncls + class sums its 2^n_held partials in place as a FORGET on the held bits, in ascending
// order of the bit -- cut_reduce()'s sequence, one barrier per bit -- and writes z = P[0] * scale.  It is launched on the same stream after the sweep
// kernel: stream order is the only synchronisation, there are no flags and no atomics.
//
// A state vector beyond 64 KiB (width 14: 128 KiB, one workgroup per CU) needs the kernel's dynamic-LDS limit raised; the launch does that once per
// device and answers hipErrorInvalidValue where the runtime refuses, which the entry point reports as QECMC_ERR_UNSUPPORTED.
#include "class_sweep_cut.hpp"

#include <mutex>

namespace qecmc {

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_sweep_cut(const SweepCutArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                     const uint32_t *__restrict__ reps, double *__restrict__ P)
{
    extern __shared__ double sweep_cut_lds[];                 // [2^width]
    const uint32_t tid = threadIdx.x, threads = blockDim.x, pair = blockIdx.x >> a.n_held, hbits = blockIdx.x & ((1u << a.n_held) - 1u);
    const uint32_t *rep = reps + (size_t)pair * (size_t)a.W;
    if (tid == 0) sweep_cut_lds[0] = 1.0;
    __syncthreads();
    for (int o = 0; o < a.n_ops; ++o) {
        const uint32_t w0 = ops[4 * o], mask = ops[4 * o + 1];
        const uint32_t kind = w0 & 15u, slot = (w0 >> 4) & 15u, top = (w0 >> 12) & 31u, bit = 1u << slot;
        if (kind == sweep::kClose) {
            const uint32_t pairs = ops[4 * o + 2], q = ops[4 * o + 3];
            uint32_t word = rep[q >> 4];
            for (uint32_t rest = hbits; rest; rest &= rest - 1u) word ^= held[(uint32_t)(__ffs(rest) - 1) * (uint32_t)a.W + (q >> 4)];
            const uint32_t cq = sweep::pauli_to_xz((word >> ((q & 15u) * 2u)) & 3u);
            for (uint32_t f = tid; f < (1u << top); f += threads) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                const double lo = (idx & 1u) ? a.wxz[1] : a.wxz[0], hi = (idx & 1u) ? a.wxz[3] : a.wxz[2];
                sweep_cut_lds[f] = sweep_cut_lds[f] * ((idx & 2u) ? hi : lo);
            }
        } else {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += threads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                if (kind == sweep::kIntro) sweep_cut_lds[f | bit] = sweep_cut_lds[f];
                else sweep_cut_lds[f] = sweep_cut_lds[f] + sweep_cut_lds[f | bit];
            }
        }
        __syncthreads();
    }
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

// the dynamic-LDS limit of k_class_sweep_cut on the current device, raised once to kCutLdsBudget where a plan of this width needs more than the default
// window; hipErrorInvalidValue where the runtime does not grant it
hipError_t class_sweep_cut_allow_lds(int width)
{
    if (!sweep::cut_fits(width)) return hipErrorInvalidValue;
    if (sweep::lds_carve(width).bytes <= sweep::kLdsBudget) return hipSuccess;
    constexpr int kDevices = 64;
    static std::mutex mu;
    static signed char state[kDevices] = {};                  // 0: not asked, 1: granted, -1: refused
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= kDevices) return hipErrorInvalidValue;
    std::lock_guard<std::mutex> g(mu);
    if (state[dev] == 0) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_class_sweep_cut), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sweep::kCutLdsBudget);
        if (e != hipSuccess) (void)hipGetLastError();         // (the refusal is reported by value; it is not left behind as the thread's last error)
        state[dev] = e == hipSuccess ? 1 : -1;
    }
    return state[dev] == 1 ? hipSuccess : hipErrorInvalidValue;
}

hipError_t launch_class_sweep_cut(const SweepCutArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, double *P, double *z, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if ((a.ncls != 4 && a.ncls != 16) || !sweep::cut_fits(a.width) || a.W < 1 || a.n_ops < 1 || a.n_held < 0 || a.n_held > sweep::kMaxHeld ||
        a.S > sweep::cut_launch_group(a.S, a.ncls, a.n_held))
        return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_sweep_cut_allow_lds(a.width)) return e;
    const uint32_t pairs = a.S * (uint32_t)a.ncls;
    hipLaunchKernelGGL(k_class_sweep_cut, dim3(pairs << a.n_held), dim3(sweep::cut_threads(a.width)), carve.bytes, stream, a, ops, held, reps, P);
    if (hipError_t e = hipGetLastError()) return e;
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
