// qecmc_class_minplus_chains: the traceback of class_minplus_trace.hpp.  The partials are k_class_minplus's (class_minplus.hip), unchanged; the three
// kernels here run after it on the same stream.  Stream order is the only synchronisation: no atomics, no flags, no scratch, no static LDS.
//
// k_minplus_pick: one wave per (syndrome, class) pair, between the sweep and the reduce -- which folds the partials in place.  Every lane walks its
// share of the 2^n_held partials and keeps the least cost << 12 | h (kMaxHeld = 12, a cost is below 2^16); a butterfly of shuffles leaves the least
// of the wave in every lane: the least cost, and the lowest h that reaches it.  pick[pair] leaves through one vector store.
//
// k_minplus_trace: grid = pairs, block and dynamic LDS as k_class_minplus (cut_threads, lds_carve), hbits = pick[pair]; the body is
// minplus::trace_sweep (class_minplus_trace.hpp), which k_minplus_trace_site shares: the CLOSE and INTRO passes of class_sweep_ops.hpp and a FORGET
// that ballots its decisions into D.  The four costs are kernel arguments.  Dirty LDS and a dirty D are allowed: the walk reads only bits of live f,
// which this kernel wrote.
//
// k_minplus_walk: one wave per pair, launched after the trace kernel, so the decision words are read by a kernel that never wrote them.  The walk is
// wave-uniform -- f, fi and the op words are the same in every lane --; lane w < W carries chain word w, and at the end the lanes unpack the words to
// uint8[nq] through shuffles and vector stores.
//
// The 128 KiB state vector (width 14) needs the dynamic-LDS limit of k_minplus_trace raised: that limit is an attribute of each kernel.
#include "class_minplus_trace.hpp"

namespace qecmc {

constexpr int kWave = (int)minplus::kTraceWave;
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
    minplus::trace_sweep(trace_lds, t, ops, held, reps, pick, D, sweep::UniformFour<uint32_t>{t.m.cxz});
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

hipError_t class_minplus_trace_allow_lds(int width)
{
    static LdsOptIn opt;
    return cut_allow_lds(reinterpret_cast<const void *>(k_minplus_trace), opt, width);
}

static bool trace_args_ok(const MinplusArgs &a)
{
    return sweep::cut_args_ok(a.S, a.ncls, a.width, a.W, a.n_ops, a.n_held) && a.W <= kWave;
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
