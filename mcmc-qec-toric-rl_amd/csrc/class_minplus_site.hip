// qecmc_class_minplus_site, qecmc_class_minplus_chains_site: the (min, +, count) sweep and its traceback under a cost per (syndrome, qubit)
// (class_minplus_site.hpp).
//
// Each kernel is its sibling's -- k_class_minplus (class_minplus.hip), k_minplus_trace (class_minplus_trace.hip) -- op for op, entry for entry,
// barrier for barrier and ballot for ballot; those comments hold here.  The one difference is in CLOSE: the four costs are not kernel arguments but
// the four bytes of the word cw[(per_syndrome ? syndrome : 0) * nq + q], in (x, z) order.  The syndrome comes from the block index alone --
// (blockIdx.x >> n_held) / ncls in the sweep kernel, blockIdx.x / ncls in the trace kernel -- and q from the plan, so the address is wave-uniform:
// the word arrives by one scalar load per CLOSE, next to the scalar loads of the op's words, and no lane carries the table.  The sibling's two
// selects per entry become a shift by 8 * idx and a mask; the add to the upper 16 bits follows as there.  Values leave through vector stores.  No
// atomics, no flags, no scratch, no static LDS.
//
// The partials are reduced by k_class_minplus_reduce, the assignment is picked by k_minplus_pick and the chain is walked by k_minplus_walk, the
// siblings' own kernels through their own launch functions (launch_class_minplus_reduce, launch_minplus_pick, launch_minplus_walk): none of the
// three looks at a cost.  Stream order is the only synchronisation.
//
// The 128 KiB state vector (width 14) needs the dynamic-LDS limit raised, and that limit is an attribute of each kernel: either kernel here has its
// own *_allow_lds, written as the siblings' are.
#include "class_minplus_site.hpp"

#include <mutex>

namespace qecmc {

constexpr int kSiteWave = 64;

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_minplus_site(const MinplusSiteArgs s, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                        const uint32_t *__restrict__ reps, const uint32_t *__restrict__ cw, uint64_t *__restrict__ P)
{
    extern __shared__ uint64_t minplus_site_lds[];            // [2^width]
    const MinplusArgs &a = s.t.m;
    const uint32_t tid = threadIdx.x, threads = blockDim.x, pair = blockIdx.x >> a.n_held, hbits = blockIdx.x & ((1u << a.n_held) - 1u);
    const uint32_t *rep = reps + (size_t)pair * (size_t)a.W;
    const uint32_t *row = cw + (size_t)(s.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)s.t.nq;
    if (tid == 0) minplus_site_lds[0] = 1ull;                 // (0, 1)
    __syncthreads();
    for (int o = 0; o < a.n_ops; ++o) {
        const uint32_t w0 = ops[4 * o], mask = ops[4 * o + 1];
        const uint32_t kind = w0 & 15u, slot = (w0 >> 4) & 15u, top = (w0 >> 12) & 31u, bit = 1u << slot;
        if (kind == sweep::kClose) {
            const uint32_t pairs = ops[4 * o + 2], q = ops[4 * o + 3];
            uint32_t word = rep[q >> 4];
            for (uint32_t rest = hbits; rest; rest &= rest - 1u) word ^= held[(uint32_t)(__ffs(rest) - 1) * (uint32_t)a.W + (q >> 4)];
            const uint32_t cq = sweep::pauli_to_xz((word >> ((q & 15u) * 2u)) & 3u);
            const uint32_t costs = row[q];
            for (uint32_t f = tid; f < (1u << top); f += threads) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                minplus_site_lds[f] = minplus_site_lds[f] + ((uint64_t)minplus::site_cost(costs, idx) << minplus::kCountBits);
            }
        } else {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += threads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                if (kind == sweep::kIntro) minplus_site_lds[f | bit] = minplus_site_lds[f];
                else minplus_site_lds[f] = minplus::mp_combine(minplus_site_lds[f], minplus_site_lds[f | bit]);
            }
        }
        __syncthreads();
    }
    if (tid == 0) P[blockIdx.x] = minplus_site_lds[0];
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_minplus_trace_site(const MinplusSiteArgs s, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                        const uint32_t *__restrict__ reps, const uint32_t *__restrict__ cw,
                                                                        const uint32_t *__restrict__ pick, uint64_t *__restrict__ D)
{
    extern __shared__ uint64_t trace_site_lds[];              // [2^width]
    const MinplusTraceArgs &t = s.t;
    const MinplusArgs &a = t.m;
    const uint32_t tid = threadIdx.x, threads = blockDim.x, lane = tid & (kSiteWave - 1u), pair = blockIdx.x, hbits = pick[pair] & ((1u << a.n_held) - 1u);
    const uint32_t *rep = reps + (size_t)pair * (size_t)a.W;
    const uint32_t *row = cw + (size_t)(s.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)t.nq;
    uint64_t *mine = D + (size_t)pair * (size_t)t.n_forget * (size_t)t.words_per_forget;
    int fi = 0;
    if (tid == 0) trace_site_lds[0] = 1ull;                   // (0, 1)
    __syncthreads();
    for (int o = 0; o < a.n_ops; ++o) {
        const uint32_t w0 = ops[4 * o], mask = ops[4 * o + 1];
        const uint32_t kind = w0 & 15u, slot = (w0 >> 4) & 15u, top = (w0 >> 12) & 31u, bit = 1u << slot;
        if (kind == sweep::kClose) {
            const uint32_t pairs = ops[4 * o + 2], q = ops[4 * o + 3];
            uint32_t word = rep[q >> 4];
            for (uint32_t rest = hbits; rest; rest &= rest - 1u) word ^= held[(uint32_t)(__ffs(rest) - 1) * (uint32_t)a.W + (q >> 4)];
            const uint32_t cq = sweep::pauli_to_xz((word >> ((q & 15u) * 2u)) & 3u);
            const uint32_t costs = row[q];
            for (uint32_t f = tid; f < (1u << top); f += threads) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                trace_site_lds[f] = trace_site_lds[f] + ((uint64_t)minplus::site_cost(costs, idx) << minplus::kCountBits);
            }
        } else if (kind == sweep::kIntro) {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += threads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                trace_site_lds[f | bit] = trace_site_lds[f];
            }
        } else {
            const uint32_t n_h = 1u << (top - 1u);
            if (fi < t.n_forget)                              // (always: the plan counts its FORGETs; a stream that does not cannot leave its rows of D)
                for (uint32_t h0 = tid - lane; h0 < n_h; h0 += threads) {          // whole waves: h0 is wave-uniform
                    const uint32_t h = h0 + lane, f = sweep::insert_zero(h, slot);
                    const bool live = h < n_h && !(f & ~mask);
                    bool take = false;
                    if (live) {
                        const uint64_t off = trace_site_lds[f], on = trace_site_lds[f | bit];
                        take = (on >> minplus::kCountBits) < (off >> minplus::kCountBits);     // strict: a tie leaves the generator off
                        trace_site_lds[f] = minplus::mp_combine(off, on);
                    }
                    const uint64_t word = __ballot(take);
                    if (lane == 0) mine[(size_t)fi * (size_t)t.words_per_forget + (h0 >> 6)] = word;
                }
            ++fi;
        }
        __syncthreads();
    }
}

// class_minplus_allow_lds()'s rule for one kernel of this unit: the dynamic-LDS limit raised once per device, hipErrorInvalidValue where refused
static hipError_t site_allow_lds(const void *kernel, signed char *state, std::mutex &mu, int devices, int width)
{
    if (!sweep::cut_fits(width)) return hipErrorInvalidValue;
    if (sweep::lds_carve(width).bytes <= sweep::kLdsBudget) return hipSuccess;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= devices) return hipErrorInvalidValue;
    std::lock_guard<std::mutex> g(mu);
    if (state[dev] == 0) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sweep::kCutLdsBudget);
        if (e != hipSuccess) (void)hipGetLastError();         // (the refusal is reported by value; it is not left behind as the thread's last error)
        state[dev] = e == hipSuccess ? 1 : -1;
    }
    return state[dev] == 1 ? hipSuccess : hipErrorInvalidValue;
}

hipError_t class_minplus_site_allow_lds(int width)
{
    constexpr int kDevices = 64;
    static std::mutex mu;
    static signed char state[kDevices] = {};                  // 0: not asked, 1: granted, -1: refused
    return site_allow_lds(reinterpret_cast<const void *>(k_class_minplus_site), state, mu, kDevices, width);
}

hipError_t class_minplus_trace_site_allow_lds(int width)
{
    constexpr int kDevices = 64;
    static std::mutex mu;
    static signed char state[kDevices] = {};                  // 0: not asked, 1: granted, -1: refused
    return site_allow_lds(reinterpret_cast<const void *>(k_minplus_trace_site), state, mu, kDevices, width);
}

// what both launches ask of their arguments: minplus_args_ok()'s and trace_args_ok()'s conditions, a table, a qubit count that the packed words hold
static bool site_args_ok(const MinplusSiteArgs &s, const uint32_t *cw)
{
    const MinplusArgs &a = s.t.m;
    return (a.ncls == 4 || a.ncls == 16) && sweep::cut_fits(a.width) && a.W >= 1 && a.W <= kSiteWave && a.n_ops >= 1 && a.n_held >= 0 && a.n_held <= sweep::kMaxHeld &&
           a.shift >= 0 && a.shift < minplus::kCountBits && a.S <= sweep::cut_launch_group(a.S, a.ncls, a.n_held) && cw && s.t.nq >= 1 && s.t.nq <= 16 * a.W &&
           (s.per_syndrome == 0 || s.per_syndrome == 1);
}

hipError_t launch_class_minplus_site_sweep(const MinplusSiteArgs &s, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *cw, uint64_t *P,
                                           hipStream_t stream)
{
    const MinplusArgs &a = s.t.m;
    if (a.S == 0) return hipSuccess;
    if (!site_args_ok(s, cw)) return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_minplus_site_allow_lds(a.width)) return e;
    hipLaunchKernelGGL(k_class_minplus_site, dim3((a.S * (uint32_t)a.ncls) << a.n_held), dim3(sweep::cut_threads(a.width)), carve.bytes, stream, s, ops, held, reps, cw, P);
    return hipGetLastError();
}

hipError_t launch_minplus_trace_site(const MinplusSiteArgs &s, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *cw, const uint32_t *pick,
                                     uint64_t *D, hipStream_t stream)
{
    const MinplusTraceArgs &t = s.t;
    const MinplusArgs &a = t.m;
    if (a.S == 0) return hipSuccess;
    if (!site_args_ok(s, cw) || t.n_forget < 1 || t.words_per_forget != minplus::trace_words_per_forget(a.width) ||
        (uint64_t)a.S * (uint64_t)a.ncls * (uint64_t)t.n_forget * (uint64_t)t.words_per_forget * 8ull > minplus::kTraceWorkspaceBytes)
        return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_minplus_trace_site_allow_lds(a.width)) return e;
    hipLaunchKernelGGL(k_minplus_trace_site, dim3(a.S * (uint32_t)a.ncls), dim3(sweep::cut_threads(a.width)), carve.bytes, stream, s, ops, held, reps, cw, pick, D);
    return hipGetLastError();
}

}  // namespace qecmc
