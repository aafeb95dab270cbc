// qecmc_class_minplus: the (min, +, count) sweep of class_minplus.hpp.
//
// k_class_minplus: grid and block as k_class_sweep_cut (class_sweep_cut.hip) -- workgroup blockIdx.x = ((syndrome * ncls + class) << n_held) + h sweeps
// one representative under one assignment h of the held generators, blockDim = cut_threads(width).  The state vector is uint64_t[2^width] in dynamic
// LDS, one packed (cost, count) entry where the sibling keeps a double; dirty LDS is allowed, only A[0] = (0, 1) is set up.  The op loop is
// minplus_one()'s, entry for entry: INTRO copies, CLOSE adds the cost of the qubit's Pauli to the upper 16 bits, FORGET is mp_combine; one barrier per
// op.  The plan, the representative and the held words are read under wave-uniform control flow (scalar loads); the four costs are kernel arguments.
// The packed partial leaves through one vector store, P[blockIdx.x].
//
// k_class_minplus_reduce: workgroup blockIdx.x = syndrome * ncls + class combines its 2^n_held partials in place with mp_combine -- associative and
// commutative, so the order is free; it folds the held bits in ascending order, one barrier per bit --, then unpacks, shifts the count by
// n_gen - rank, reports a saturated count as 0 and writes cost_out and count_out.  It also runs when n_held = 0.  It is launched on the same stream
// after the sweep kernel: stream order is the only synchronisation, there are no flags and no atomics.  Either kernel has a host function of its own
// (launch_class_minplus_sweep, launch_class_minplus_reduce; launch_class_minplus calls both): the traceback (class_minplus_trace.hip) reads the partials
// between the two.
//
// A state vector beyond 64 KiB (width 14: 128 KiB, one workgroup per CU) needs the kernel's dynamic-LDS limit raised.  That limit is an attribute of
// each kernel: class_sweep_cut_allow_lds raises it for k_class_sweep_cut only, so this unit asks for its own kernel, once per device, and answers
// hipErrorInvalidValue where the runtime refuses, which the entry point reports as QECMC_ERR_UNSUPPORTED.
#include "class_minplus.hpp"

#include <mutex>

namespace qecmc {

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_minplus(const MinplusArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                   const uint32_t *__restrict__ reps, uint64_t *__restrict__ P)
{
    extern __shared__ uint64_t minplus_lds[];                 // [2^width]
    const uint32_t tid = threadIdx.x, threads = blockDim.x, pair = blockIdx.x >> a.n_held, hbits = blockIdx.x & ((1u << a.n_held) - 1u);
    const uint32_t *rep = reps + (size_t)pair * (size_t)a.W;
    if (tid == 0) minplus_lds[0] = 1ull;                      // (0, 1)
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
                const uint32_t lo = (idx & 1u) ? a.cxz[1] : a.cxz[0], hi = (idx & 1u) ? a.cxz[3] : a.cxz[2];
                minplus_lds[f] = minplus_lds[f] + ((uint64_t)((idx & 2u) ? hi : lo) << minplus::kCountBits);
            }
        } else {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += threads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                if (kind == sweep::kIntro) minplus_lds[f | bit] = minplus_lds[f];
                else minplus_lds[f] = minplus::mp_combine(minplus_lds[f], minplus_lds[f | bit]);
            }
        }
        __syncthreads();
    }
    if (tid == 0) P[blockIdx.x] = minplus_lds[0];
}

__global__ __launch_bounds__(sweep::kThreads) void k_class_minplus_reduce(const MinplusArgs a, uint64_t *P, uint32_t *__restrict__ cost_out, uint64_t *__restrict__ count_out)
{
    uint64_t *mine = P + ((size_t)blockIdx.x << a.n_held);
    for (int j = 0; j < a.n_held; ++j) {
        for (uint32_t k = threadIdx.x; k < (1u << (a.n_held - 1 - j)); k += sweep::kThreads) {
            const uint32_t h = k << (j + 1);
            mine[h] = minplus::mp_combine(mine[h], mine[h | (1u << j)]);
        }
        __syncthreads();                                      // (the next bit reads what other lanes of this workgroup wrote)
    }
    if (threadIdx.x == 0) {
        uint32_t cost;
        uint64_t count;
        minplus::mp_unpack(mine[0], a.shift, &cost, &count);
        cost_out[blockIdx.x] = cost;
        count_out[blockIdx.x] = count;
    }
}

// the dynamic-LDS limit of k_class_minplus on the current device, raised once to kCutLdsBudget where a plan of this width needs more than the default
// window; hipErrorInvalidValue where the runtime does not grant it
hipError_t class_minplus_allow_lds(int width)
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
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_class_minplus), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sweep::kCutLdsBudget);
        if (e != hipSuccess) (void)hipGetLastError();         // (the refusal is reported by value; it is not left behind as the thread's last error)
        state[dev] = e == hipSuccess ? 1 : -1;
    }
    return state[dev] == 1 ? hipSuccess : hipErrorInvalidValue;
}

static bool minplus_args_ok(const MinplusArgs &a)
{
    return (a.ncls == 4 || a.ncls == 16) && sweep::cut_fits(a.width) && a.W >= 1 && a.n_ops >= 1 && a.n_held >= 0 && a.n_held <= sweep::kMaxHeld && a.shift >= 0 &&
           a.shift < minplus::kCountBits && a.S <= sweep::cut_launch_group(a.S, a.ncls, a.n_held);
}

hipError_t launch_class_minplus_sweep(const MinplusArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, uint64_t *P, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if (!minplus_args_ok(a)) return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_minplus_allow_lds(a.width)) return e;
    hipLaunchKernelGGL(k_class_minplus, dim3((a.S * (uint32_t)a.ncls) << a.n_held), dim3(sweep::cut_threads(a.width)), carve.bytes, stream, a, ops, held, reps, P);
    return hipGetLastError();
}

hipError_t launch_class_minplus_reduce(const MinplusArgs &a, uint64_t *P, uint32_t *cost_out, uint64_t *count_out, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if (!minplus_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_class_minplus_reduce, dim3(a.S * (uint32_t)a.ncls), dim3(sweep::kThreads), 0, stream, a, P, cost_out, count_out);
    return hipGetLastError();
}

hipError_t launch_class_minplus(const MinplusArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, uint64_t *P, uint32_t *cost_out, uint64_t *count_out,
                                hipStream_t stream)
{
    if (hipError_t e = launch_class_minplus_sweep(a, ops, held, reps, P, stream)) return e;
    return launch_class_minplus_reduce(a, P, cost_out, count_out, stream);
}

}  // namespace qecmc
