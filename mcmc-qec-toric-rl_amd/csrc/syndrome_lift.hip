// qecmc_chains_from_syndromes: the lift-and-descend body of syndrome_lift.hpp with one lane per syndrome.  A workgroup is one wavefront of 64
// syndromes; the states live in LDS in the lane-private layout of ladder_kernel.hpp (word w of lane l at [w][l]: the 64 lanes of an access hit 64
// banks), so no per-lane register array is indexed dynamically.  The table row of a cell and the generator of a descent step are the same for all
// 64 lanes: their addresses are formed from kernel arguments and loop counters alone, and the const __restrict__ tables are read with scalar loads.
// A lane whose cell is clear, or whose generator does not lower its count, is predicated off.
#include "syndrome_lift.hpp"

#include <mutex>

namespace qecmc {

namespace {

struct LdsState {
    uint32_t *col;                                            // this lane's column of [W][64]
    __device__ __forceinline__ uint32_t get(int w) const { return col[w * 64]; }
    __device__ __forceinline__ void set(int w, uint32_t v) { col[w * 64] = v; }
    __device__ __forceinline__ bool any(bool b) const { return __ballot(b) != 0ull; }
};

}  // namespace

__global__ __launch_bounds__(64) void k_syndrome_lift(const LiftArgs a, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ gen,
                                                      const uint8_t *__restrict__ defects, uint8_t *__restrict__ chains, uint8_t *__restrict__ status,
                                                      int32_t *__restrict__ weight)
{
    extern __shared__ uint32_t lift_lds[];                    // [W][64]
    const uint32_t lane = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * 64u, s = first + lane;
    const bool live = s < a.N;
    LdsState st{lift_lds + lane};
    int stat = 0, wgt = 0;
    lift::lift_body(st, rows, gen, a.n_cells, a.W, a.nq, a.n_gen, live ? defects + s * (uint64_t)a.n_cells : nullptr, a.descend, stat, wgt);
    if (live) {
        if (status) status[s] = (uint8_t)stat;
        if (weight) weight[s] = wgt;
    }
    __syncthreads();
    // the workgroup's chains are one contiguous run of bytes: lane l writes bytes l, l + 64, ... of it (coalesced), each from its syndrome's column
    const uint64_t n_here = a.N - first < 64u ? a.N - first : 64u;
    const uint32_t total = (uint32_t)n_here * (uint32_t)a.nq, nq = (uint32_t)a.nq;
    uint8_t *out = chains + first * (uint64_t)nq;
    for (uint32_t i = lane; i < total; i += 64u) {
        const uint32_t syn = i / nq, q = i - syn * nq;
        out[i] = (uint8_t)((lift_lds[(q >> 4) * 64u + syn] >> ((q & 15u) * 2u)) & 3u);
    }
}

// the dynamic-LDS limit of k_syndrome_lift on the current device: beyond the default 64 KiB window it is raised ONCE per device, to kServiceLdsMax (what the
// largest accepted lattice needs), under a mutex -- never per launch with the launch's own size, which would let one host thread lower the limit
// between another thread's request and its launch.  hipErrorInvalidValue where the runtime does not grant it
static hipError_t lift_allow_lds(size_t lds)
{
    if (lds <= 64 * 1024) return hipSuccess;
    constexpr int kDevices = 64;
    static std::mutex mu;
    static signed char state[kDevices] = {};                  // 0: not asked, 1: granted, -1: refused
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= kDevices) return hipErrorInvalidValue;
    std::lock_guard<std::mutex> g(mu);
    if (state[dev] == 0) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_syndrome_lift), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kServiceLdsMax);
        if (e != hipSuccess) (void)hipGetLastError();         // (the refusal is reported by value; it is not left behind as the thread's last error)
        state[dev] = e == hipSuccess ? 1 : -1;
    }
    return state[dev] == 1 ? hipSuccess : hipErrorInvalidValue;
}

hipError_t launch_syndrome_lift(const LiftArgs &a, const uint32_t *rows, const uint32_t *gen, const uint8_t *defects, uint8_t *chains, uint8_t *status,
                                int32_t *weight, hipStream_t stream)
{
    if (a.N == 0) return hipSuccess;
    const size_t lds = (size_t)a.W * 64u * sizeof(uint32_t);
    const uint64_t grid = (a.N + 63u) / 64u;
    if (lds > kServiceLdsMax || grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (hipError_t e = lift_allow_lds(lds)) return e;
    hipLaunchKernelGGL(k_syndrome_lift, dim3((unsigned)grid), dim3(64), lds, stream, a, rows, gen, defects, chains, status, weight);
    return hipGetLastError();
}

}  // namespace qecmc
