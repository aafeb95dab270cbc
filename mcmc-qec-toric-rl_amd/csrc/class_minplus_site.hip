// qecmc_class_minplus_site, qecmc_class_minplus_chains_site: the (min, +, count) sweep and its traceback under a cost per (syndrome, qubit)
// (class_minplus_site.hpp).
//
// Each kernel has its sibling's grid, block and write-out -- k_class_minplus (class_minplus.hip), k_minplus_trace (class_minplus_trace.hip) -- and its
// body: the op loop of class_sweep_ops.hpp, minplus::trace_sweep.  What is theirs is the factor source of a CLOSE: the four costs are not kernel
// arguments but the four bytes of the word cw[(per_syndrome ? syndrome : 0) * nq + q], in (x, z) order.  The syndrome comes from the block index
// alone -- (blockIdx.x >> n_held) / ncls in the sweep kernel, blockIdx.x / ncls in the trace kernel -- and q from the plan, so the address is
// wave-uniform: the word arrives by one scalar load per CLOSE, next to the scalar loads of the op's words, and no lane carries the table.  The
// sibling's two selects per entry become a shift by 8 * idx and a mask; the add to the upper 16 bits follows as there.  Values leave through vector
// stores.  No atomics, no flags, no scratch, no static LDS.
//
// The partials are reduced by k_class_minplus_reduce, the assignment is picked by k_minplus_pick and the chain is walked by k_minplus_walk, the
// siblings' own kernels through their own launch functions (launch_class_minplus_reduce, launch_minplus_pick, launch_minplus_walk): none of the
// three looks at a cost.  Stream order is the only synchronisation.
//
// The 128 KiB state vector (width 14) needs the dynamic-LDS limit raised, and that limit is an attribute of each kernel: either kernel here has its
// own *_allow_lds over cut_allow_lds (class_sweep_cut.hpp).
#include "class_minplus_site.hpp"

namespace qecmc {

constexpr int kSiteWave = (int)minplus::kTraceWave;

using minplus::SiteCosts;

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_minplus_site(const MinplusSiteArgs s, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                        const uint32_t *__restrict__ reps, const uint32_t *__restrict__ cw, uint64_t *__restrict__ P)
{
    extern __shared__ uint64_t minplus_site_lds[];            // [2^width]
    const MinplusArgs &a = s.t.m;
    const uint32_t tid = threadIdx.x, pair = blockIdx.x >> a.n_held, hbits = blockIdx.x & ((1u << a.n_held) - 1u);
    const uint32_t *row = cw + (size_t)(s.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)s.t.nq;
    if (tid == 0) minplus_site_lds[0] = 1ull;                 // (0, 1)
    __syncthreads();
    sweep::op_loop<sweep::NarrowOps, minplus::MinPlus>(minplus_site_lds, ops, 0u, (uint32_t)a.n_ops, tid, blockDim.x,
                                                       sweep::HeldRep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W}, SiteCosts{row});
    if (tid == 0) P[blockIdx.x] = minplus_site_lds[0];
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_minplus_trace_site(const MinplusSiteArgs s, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                        const uint32_t *__restrict__ reps, const uint32_t *__restrict__ cw,
                                                                        const uint32_t *__restrict__ pick, uint64_t *__restrict__ D)
{
    extern __shared__ uint64_t trace_site_lds[];              // [2^width]
    const uint32_t *row = cw + (size_t)(s.per_syndrome ? blockIdx.x / (uint32_t)s.t.m.ncls : 0u) * (size_t)s.t.nq;
    minplus::trace_sweep(trace_site_lds, s.t, ops, held, reps, pick, D, SiteCosts{row});
}

hipError_t class_minplus_site_allow_lds(int width)
{
    static LdsOptIn opt;
    return cut_allow_lds(reinterpret_cast<const void *>(k_class_minplus_site), opt, width);
}

hipError_t class_minplus_trace_site_allow_lds(int width)
{
    static LdsOptIn opt;
    return cut_allow_lds(reinterpret_cast<const void *>(k_minplus_trace_site), opt, width);
}

// what both launches ask of their arguments: minplus_args_ok()'s and trace_args_ok()'s conditions, a table, a qubit count that the packed words hold
static bool site_args_ok(const MinplusSiteArgs &s, const uint32_t *cw)
{
    const MinplusArgs &a = s.t.m;
    return sweep::cut_args_ok(a.S, a.ncls, a.width, a.W, a.n_ops, a.n_held) && a.W <= kSiteWave && a.shift >= 0 && a.shift < minplus::kCountBits && cw && s.t.nq >= 1 &&
           s.t.nq <= 16 * a.W && (s.per_syndrome == 0 || s.per_syndrome == 1);
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
