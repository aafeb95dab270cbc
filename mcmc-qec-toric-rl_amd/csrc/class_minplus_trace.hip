// qecmc_class_minplus_chains: the traceback of class_minplus_trace.hpp.  The partials are k_class_minplus's (class_minplus.hip), unchanged; the three
// kernels here run after it on the same stream.  Stream order is the only synchronisation: no atomics, no flags, no scratch, no static LDS.
//
// k_minplus_pick: one wave per (syndrome, class) pair, between the sweep and the reduce -- which folds the partials in place.  Every lane walks its
// share of the 2^n_held partials and keeps the least cost << 12 | h (kMaxHeld = 12, a cost is below 2^16); a butterfly of shuffles leaves the least
// of the wave in every lane: the least cost, and the lowest h that reaches it.  pick[pair] leaves through one vector store.
//
// k_minplus_trace: grid = pairs, block and dynamic LDS as k_class_minplus (cut_threads, lds_carve), hbits = pick[pair], the op loop k_class_minplus's
// entry for entry.  A FORGET walks its h in whole waves -- the loop bound is wave-uniform, a lane past the bound or on a dead f stays in the wave and
// contributes 0 -- so that __ballot(live && take) is the 64 decisions of h0 .. h0 + 63; the first lane of the wave stores it to
// D[pair][fi][h0 >> 6] with one 64-bit vector store.  Where 2^(top - 1) < 64 the one word is word 0 of wave 0.  The LDS accesses stay behind the
// live mask.  Dirty LDS and a dirty D are allowed: the walk reads only bits of live f, which this kernel wrote.
//
// k_minplus_walk: one wave per pair, launched after the trace kernel, so the decision words are read by a kernel that never wrote them.  The walk is
// wave-uniform -- f, fi and the op words are the same in every lane --; lane w < W carries chain word w, and at the end the lanes unpack the words to
// uint8[nq] through shuffles and vector stores.
//
// The 128 KiB state vector (width 14) needs the dynamic-LDS limit of k_minplus_trace raised: that limit is an attribute of each kernel.
#include "class_minplus_trace.hpp"

#include <mutex>

namespace qecmc {

constexpr int kWave = 64;
static_assert(sweep::kMaxHeld <= 12 && 11 * 11 * minplus::kMaxCost < (1u << 16), "cost << 12 | h fits 32 bits");

__global__ __launch_bounds__(kWave) void k_minplus_pick(const MinplusArgs a, const uint64_t *__restrict__ P, uint32_t *__restrict__ pick)
{
    const uint64_t *mine = P + ((size_t)blockIdx.x << a.n_held);
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t h = threadIdx.x; h < (1u << a.n_held); h += kWave) {
        const uint32_t key = ((uint32_t)(mine[h] >> minplus::kCountBits) << 12) | h;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)best, d, kWave);
        best = other < best ? other : best;
    }
    if (threadIdx.x == 0) pick[blockIdx.x] = best & 0xFFFu;
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_minplus_trace(const MinplusTraceArgs t, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                   const uint32_t *__restrict__ reps, const uint32_t *__restrict__ pick, uint64_t *__restrict__ D)
{
    extern __shared__ uint64_t trace_lds[];                   // [2^width]
    const MinplusArgs &a = t.m;
    const uint32_t tid = threadIdx.x, threads = blockDim.x, lane = tid & (kWave - 1u), pair = blockIdx.x, hbits = pick[pair] & ((1u << a.n_held) - 1u);
    const uint32_t *rep = reps + (size_t)pair * (size_t)a.W;
    uint64_t *mine = D + (size_t)pair * (size_t)t.n_forget * (size_t)t.words_per_forget;
    int fi = 0;
    if (tid == 0) trace_lds[0] = 1ull;                        // (0, 1)
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
                trace_lds[f] = trace_lds[f] + ((uint64_t)((idx & 2u) ? hi : lo) << minplus::kCountBits);
            }
        } else if (kind == sweep::kIntro) {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += threads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                trace_lds[f | bit] = trace_lds[f];
            }
        } else {
            const uint32_t n_h = 1u << (top - 1u);
            if (fi < t.n_forget)                              // (always: the plan counts its FORGETs; a stream that does not cannot leave its rows of D)
                for (uint32_t h0 = tid - lane; h0 < n_h; h0 += threads) {          // whole waves: h0 is wave-uniform
                    const uint32_t h = h0 + lane, f = sweep::insert_zero(h, slot);
                    const bool live = h < n_h && !(f & ~mask);
                    bool take = false;
                    if (live) {
                        const uint64_t off = trace_lds[f], on = trace_lds[f | bit];
                        take = (on >> minplus::kCountBits) < (off >> minplus::kCountBits);     // strict: a tie leaves the generator off
                        trace_lds[f] = minplus::mp_combine(off, on);
                    }
                    const uint64_t word = __ballot(take);
                    if (lane == 0) mine[(size_t)fi * (size_t)t.words_per_forget + (h0 >> 6)] = word;
                }
            ++fi;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kWave) void k_minplus_walk(const MinplusTraceArgs t, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                        const uint32_t *__restrict__ reps, const uint32_t *__restrict__ forget_words, const uint32_t *__restrict__ pick,
                                                        const uint64_t *__restrict__ D, uint8_t *__restrict__ chain_out)
{
    const MinplusArgs &a = t.m;
    const uint32_t lane = threadIdx.x, pair = blockIdx.x, hbits = pick[pair] & ((1u << a.n_held) - 1u);
    const uint64_t *mine = D + (size_t)pair * (size_t)t.n_forget * (size_t)t.words_per_forget;
    uint32_t chain = 0;
    if (lane < (uint32_t)a.W) {
        chain = reps[(size_t)pair * (size_t)a.W + lane];
        for (uint32_t rest = hbits; rest; rest &= rest - 1u) chain ^= held[(uint32_t)(__ffs(rest) - 1) * (uint32_t)a.W + lane];
    }
    uint32_t f = 0;
    int fi = t.n_forget;
    for (int o = a.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = ops[4 * o], kind = w0 & 15u, slot = (w0 >> 4) & 15u, bit = 1u << slot;
        if (kind == sweep::kIntro) f &= ~bit;
        else if (kind == sweep::kForget && fi > 0) {
            --fi;
            const uint32_t h = minplus::remove_bit(f, slot);
            if ((mine[(size_t)fi * (size_t)t.words_per_forget + (h >> 6)] >> (h & 63u)) & 1ull) {
                f |= bit;
                if (lane < (uint32_t)a.W) chain ^= forget_words[(size_t)fi * (size_t)a.W + lane];
            }
        }
    }
    uint8_t *out = chain_out + (size_t)pair * (size_t)t.nq;
    for (uint32_t q0 = 0; q0 < (uint32_t)t.nq; q0 += kWave) {                     // whole waves: every lane takes part in the shuffle
        const uint32_t q = q0 + lane;
        const uint32_t word = (uint32_t)__shfl((int)chain, (int)((q >> 4) & (kWave - 1u)), kWave);
        if (q < (uint32_t)t.nq) out[q] = (uint8_t)((word >> ((q & 15u) * 2u)) & 3u);
    }
}

// the dynamic-LDS limit of k_minplus_trace on the current device, raised once to kCutLdsBudget where a plan of this width needs more than the default
// window; hipErrorInvalidValue where the runtime does not grant it
hipError_t class_minplus_trace_allow_lds(int width)
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
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_minplus_trace), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sweep::kCutLdsBudget);
        if (e != hipSuccess) (void)hipGetLastError();         // (the refusal is reported by value; it is not left behind as the thread's last error)
        state[dev] = e == hipSuccess ? 1 : -1;
    }
    return state[dev] == 1 ? hipSuccess : hipErrorInvalidValue;
}

static bool trace_args_ok(const MinplusArgs &a)
{
    return (a.ncls == 4 || a.ncls == 16) && sweep::cut_fits(a.width) && a.W >= 1 && a.W <= kWave && a.n_ops >= 1 && a.n_held >= 0 && a.n_held <= sweep::kMaxHeld &&
           a.S <= sweep::cut_launch_group(a.S, a.ncls, a.n_held);
}

hipError_t launch_minplus_pick(const MinplusArgs &a, const uint64_t *P, uint32_t *pick, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if (!trace_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_minplus_pick, dim3(a.S * (uint32_t)a.ncls), dim3(kWave), 0, stream, a, P, pick);
    return hipGetLastError();
}

static bool trace_shape_ok(const MinplusTraceArgs &t)
{
    const MinplusArgs &a = t.m;
    return trace_args_ok(a) && t.n_forget >= 1 && t.words_per_forget == minplus::trace_words_per_forget(a.width) && t.nq >= 1 && t.nq <= 16 * a.W &&
           (uint64_t)a.S * (uint64_t)a.ncls * (uint64_t)t.n_forget * (uint64_t)t.words_per_forget * 8ull <= minplus::kTraceWorkspaceBytes;
}

hipError_t launch_minplus_walk(const MinplusTraceArgs &t, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *forget_words, const uint32_t *pick,
                               const uint64_t *D, uint8_t *chain_out, hipStream_t stream)
{
    const MinplusArgs &a = t.m;
    if (a.S == 0) return hipSuccess;
    if (!trace_shape_ok(t)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_minplus_walk, dim3(a.S * (uint32_t)a.ncls), dim3(kWave), 0, stream, t, ops, held, reps, forget_words, pick, D, chain_out);
    return hipGetLastError();
}

hipError_t launch_minplus_trace(const MinplusTraceArgs &t, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *forget_words, const uint32_t *pick,
                                uint64_t *D, uint8_t *chain_out, hipStream_t stream)
{
    const MinplusArgs &a = t.m;
    if (a.S == 0) return hipSuccess;
    if (!trace_shape_ok(t)) return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_minplus_trace_allow_lds(a.width)) return e;
    hipLaunchKernelGGL(k_minplus_trace, dim3(a.S * (uint32_t)a.ncls), dim3(sweep::cut_threads(a.width)), carve.bytes, stream, t, ops, held, reps, pick, D);
    if (hipError_t e = hipGetLastError()) return e;
    return launch_minplus_walk(t, ops, held, reps, forget_words, pick, D, chain_out, stream);
}

}  // namespace qecmc
