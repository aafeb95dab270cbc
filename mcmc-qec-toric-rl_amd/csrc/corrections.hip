// qecmc_corrections: the survey-pick-move-descend body of corrections.hpp with one lane per syndrome.  A workgroup is one wavefront of 64 syndromes;
// every lane holds ONE state, in LDS in the lane-private layout of k_syndrome_lift (word w of lane l at [w][l]: the 64 lanes of an access hit 64
// banks) -- the K candidates of a syndrome pass through it one after the other, and only the best index, weight and class stay in registers.  The
// rows of the logical masks, the class-move table and the generators are the same for all 64 lanes: their addresses are formed from kernel arguments
// and loop counters alone, and the const __restrict__ tables are read with scalar loads.  A lane's own class, target and chosen position only
// predicate what it does.
#include "corrections.hpp"

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

// (waves_per_eu 8: the table pointers and dimensions would otherwise take 106 scalar registers, one wave per SIMD less; the compiler then parks some of
//  them in lanes of a vector register -- no scratch either way)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) void k_corrections(const CorrectArgs a, const uint32_t *__restrict__ masks, const uint32_t *__restrict__ need,
                                                    const uint32_t *__restrict__ gen, const uint8_t *__restrict__ candidates,
                                                    const int32_t *__restrict__ target, uint8_t *__restrict__ corrections, int32_t *__restrict__ weight,
                                                    int32_t *__restrict__ source, uint8_t *__restrict__ moved, uint8_t *__restrict__ status)
{
    extern __shared__ uint32_t corr_lds[];                    // [W][64]
    const uint32_t lane = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * 64u, s = first + lane;
    const bool live = s < a.N;
    LdsState st{corr_lds + lane};
    int wgt = 0, src = 0, mov = 0, stat = 0;
    correct::correct_body(st, masks, need, gen, a.code, a.L, a.W, a.nq, a.n_gen, a.ncls, a.kinds,
                          live ? candidates + s * (uint64_t)a.K * (uint64_t)a.nq : nullptr, a.K, live ? target[s] : 0, a.place, a.descend, wgt, src, mov, stat);
    if (live) {
        if (weight) weight[s] = wgt;
        if (source) source[s] = src;
        if (moved) moved[s] = (uint8_t)mov;
        if (status) status[s] = (uint8_t)stat;
    }
    __syncthreads();
    // the workgroup's corrections are one contiguous run of bytes: lane l writes bytes l, l + 64, ... of it (coalesced), each from its syndrome's column
    const uint64_t n_here = a.N - first < 64u ? a.N - first : 64u;
    const uint32_t total = (uint32_t)n_here * (uint32_t)a.nq, nq = (uint32_t)a.nq;
    uint8_t *out = corrections + first * (uint64_t)nq;
    for (uint32_t i = lane; i < total; i += 64u) {
        const uint32_t syn = i / nq, q = i - syn * nq;
        out[i] = (uint8_t)((corr_lds[(q >> 4) * 64u + syn] >> ((q & 15u) * 2u)) & 3u);
    }
}

// the dynamic-LDS limit of k_corrections on the current device: beyond the default 64 KiB window it is raised ONCE per device, to kServiceLdsMax (what the
// largest accepted lattice needs), under a mutex -- never per launch with the launch's own size, which would let one host thread lower the limit
// between another thread's request and its launch.  hipErrorInvalidValue where the runtime does not grant it
static hipError_t corrections_allow_lds(size_t lds)
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
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_corrections), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kServiceLdsMax);
        if (e != hipSuccess) (void)hipGetLastError();         // (the refusal is reported by value; it is not left behind as the thread's last error)
        state[dev] = e == hipSuccess ? 1 : -1;
    }
    return state[dev] == 1 ? hipSuccess : hipErrorInvalidValue;
}

hipError_t launch_corrections(const CorrectArgs &a, const uint32_t *masks, const uint32_t *need, const uint32_t *gen, const uint8_t *candidates,
                              const int32_t *target, uint8_t *corrections, int32_t *weight, int32_t *source, uint8_t *moved, uint8_t *status,
                              hipStream_t stream)
{
    if (a.N == 0) return hipSuccess;
    const size_t lds = (size_t)a.W * 64u * sizeof(uint32_t);
    const uint64_t grid = (a.N + 63u) / 64u;
    if (a.K < 1 || lds > kServiceLdsMax || grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (hipError_t e = corrections_allow_lds(lds)) return e;
    hipLaunchKernelGGL(k_corrections, dim3((unsigned)grid), dim3(64), lds, stream, a, masks, need, gen, candidates, target, corrections, weight, source,
                       moved, status);
    return hipGetLastError();
}

}  // namespace qecmc
