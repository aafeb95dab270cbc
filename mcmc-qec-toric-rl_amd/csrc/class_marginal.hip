// qecmc_class_marginals, qecmc_class_marginals_site: the exact per-qubit marginals of class_marginal.hpp.  Six kernels; stream order is the only
// synchronisation: no atomics, no flags, no scratch, no static LDS.
//
// k_class_marginal_fwd, k_class_marginal_fwd_site: the grid is the jobs of the launch; block size and dynamic LDS are k_class_sweep_cut's
// (cut_threads, lds_carve).  Workgroup b sweeps job job0 + b = ((s * ncls + c) << n_held) + h forward with the INTRO and FORGET passes of
// class_sweep_ops.hpp and a CLOSE pass that, after the multiply, stores the entry with one 8-byte vector store: fwd[b][ci][f].  The unscaled partial
// leaves as k_class_sweep_cut's does, P[job0 + b]; k_class_sweep_reduce folds it into z.  The site form differs in the factor source alone.
//
// k_class_marginal_bwd, k_class_marginal_bwd_site: the same grid, B in the same LDS window, the ops in reverse, one barrier per op.  The reverse of a
// FORGET is the copy an INTRO makes under the FORGET's mask, the reverse of an INTRO the add a FORGET makes under the INTRO's mask: half_pass with
// the kind exchanged -- the same half-index walks, the same bank behaviour (slots below 4 read two 256-byte bank rows per 32-lane group).  At a CLOSE a
// lane loads the forward entry (8 bytes), stores d[f] = fwd * B[f] back over it and puts the factor onto B[f].  Unit stride in f.
//
// k_class_marginal_fold: one wave per (job, CLOSE) slice, THE RULE's 64 lanes as its 64 lanes: lane l walks f = l, l + 64, ... below the CLOSE's
// top in ascending order and adds d[f] to the sum of its idx(f), four sums in registers; then six steps v = v + v(lane ^ m), m = 32 .. 1, through
// __shfl_xor; lane 0 stores the four.  Folding inside the backward kernel would save a pass over the record, but ties the lanes of the rule to the
// 256 or 1 024 threads of that workgroup and a cross-wave step through LDS the state vector already fills at width 14; the separate wave keeps the
// rule's order free of the launch shape.
//
// k_class_marginal_combine: k_class_sweep_reduce's shape.  Workgroup blockIdx.x = s * ncls + c folds the M_h of its 2^n_held jobs in place, a FORGET
// on the held bits in ascending order of the bit with one barrier per bit, n_close * 4 sums side by side; then writes weights[s][c][q][P] =
// M[ci of q][pauli_to_xz(P)] * scale, and for a cell no CLOSE names z at the representative's byte and 0 elsewhere.
//
// The unit is built without floating-point contraction, as class_sweep_cut.hip (the Makefile's -ffp-contract=off line); doubles keep their denormals
// on this target whatever the flags.  Every product here is stored before anything is added to it.
#include "class_marginal.hpp"

namespace qecmc {

// the (x, z) index of entry f at a CLOSE: the qubit's own, folded with the pairs whose slot bit is set in f
__device__ __forceinline__ uint32_t marginal_idx(uint32_t cq, uint32_t pairs, uint32_t f)
{
    uint32_t idx = cq;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
        idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
    }
    return idx;
}

template <class Src>
__device__ __forceinline__ void marginal_forward(double *A, const MarginalArgs &a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                 const uint32_t *__restrict__ reps, double *__restrict__ fwd, double *__restrict__ P, const Src &src)
{
    const uint32_t tid = threadIdx.x, threads = blockDim.x, job = a.job0 + blockIdx.x;
    const uint32_t pair = job >> a.n_held, hbits = job & ((1u << a.n_held) - 1u);
    const sweep::HeldRep rep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W};
    double *mine = fwd + ((size_t)blockIdx.x * (size_t)a.n_close << a.width);
    int ci = 0;
    if (tid == 0) A[0] = 1.0;
    __syncthreads();
    for (uint32_t o = 0; o < (uint32_t)a.n_ops; ++o) {
        const sweep::Op<sweep::NarrowOps> op(ops, o);
        if (op.kind == sweep::kClose) {
            const uint32_t pairs = op.w[2], q = op.w[3], cq = rep(op.w, q);
            const auto row = src.row(q);
            double *keep = mine + ((size_t)ci << a.width);          // top <= width: f stays within the 2^width entries of CLOSE ci
            if (ci < a.n_close)                                      // (always: the plan counts its CLOSEs; a stream that does not cannot leave its record)
                for (uint32_t f = tid; f < (1u << op.top); f += threads) {
                    if (f & ~op.mask) continue;
                    const double v = sweep::SumProduct::close(A[f], row.at(marginal_idx(cq, pairs, f)));
                    A[f] = v;
                    keep[f] = v;
                }
            ++ci;
        } else sweep::half_pass<sweep::SumProduct>(A, tid, threads, op, op.kind);
        __syncthreads();
    }
    if (tid == 0) P[job] = A[0];
}

template <class Src>
__device__ __forceinline__ void marginal_backward(double *B, const MarginalArgs &a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                  const uint32_t *__restrict__ reps, double *__restrict__ fwd, const Src &src)
{
    const uint32_t tid = threadIdx.x, threads = blockDim.x, job = a.job0 + blockIdx.x;
    const uint32_t pair = job >> a.n_held, hbits = job & ((1u << a.n_held) - 1u);
    const sweep::HeldRep rep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W};
    double *mine = fwd + ((size_t)blockIdx.x * (size_t)a.n_close << a.width);
    int ci = a.n_close;
    if (tid == 0) B[0] = 1.0;
    __syncthreads();
    for (uint32_t o = (uint32_t)a.n_ops; o-- > 0u;) {
        const sweep::Op<sweep::NarrowOps> op(ops, o);
        if (op.kind == sweep::kClose) {
            --ci;
            const uint32_t pairs = op.w[2], q = op.w[3], cq = rep(op.w, q);
            const auto row = src.row(q);
            if (ci >= 0) {                                          // (always, as above)
                double *kept = mine + ((size_t)ci << a.width);
                for (uint32_t f = tid; f < (1u << op.top); f += threads) {
                    if (f & ~op.mask) continue;
                    const double b = B[f];
                    kept[f] = kept[f] * b;
                    B[f] = sweep::SumProduct::close(b, row.at(marginal_idx(cq, pairs, f)));
                }
            }
        } else sweep::half_pass<sweep::SumProduct>(B, tid, threads, op, op.kind == sweep::kIntro ? sweep::kForget : sweep::kIntro);
        __syncthreads();
    }
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_marginal_fwd(const MarginalArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                        const uint32_t *__restrict__ reps, double *__restrict__ fwd, double *__restrict__ P)
{
    extern __shared__ double marginal_fwd_lds[];              // [2^width]
    marginal_forward(marginal_fwd_lds, a, ops, held, reps, fwd, P, sweep::UniformFour<double>{a.wxz});
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_marginal_fwd_site(const MarginalArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                             const uint32_t *__restrict__ reps, const double *__restrict__ wq, double *__restrict__ fwd,
                                                                             double *__restrict__ P)
{
    extern __shared__ double marginal_fwd_site_lds[];         // [2^width]
    const uint32_t pair = (a.job0 + blockIdx.x) >> a.n_held;
    const double *rows = wq + (size_t)(a.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)a.nq * 4u;
    marginal_forward(marginal_fwd_site_lds, a, ops, held, reps, fwd, P, sweep::SiteFour<double>{rows});
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_marginal_bwd(const MarginalArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                        const uint32_t *__restrict__ reps, double *__restrict__ fwd)
{
    extern __shared__ double marginal_bwd_lds[];              // [2^width]
    marginal_backward(marginal_bwd_lds, a, ops, held, reps, fwd, sweep::UniformFour<double>{a.wxz});
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_marginal_bwd_site(const MarginalArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                             const uint32_t *__restrict__ reps, const double *__restrict__ wq, double *__restrict__ fwd)
{
    extern __shared__ double marginal_bwd_site_lds[];         // [2^width]
    const uint32_t pair = (a.job0 + blockIdx.x) >> a.n_held;
    const double *rows = wq + (size_t)(a.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)a.nq * 4u;
    marginal_backward(marginal_bwd_site_lds, a, ops, held, reps, fwd, sweep::SiteFour<double>{rows});
}

__global__ __launch_bounds__(marginal::kFoldLanes) void k_class_marginal_fold(const MarginalArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                              const uint32_t *__restrict__ reps, const uint32_t *__restrict__ close_op,
                                                                              const double *__restrict__ fwd, double *__restrict__ Mh)
{
    const uint32_t lane = threadIdx.x, b = blockIdx.x / (uint32_t)a.n_close, ci = blockIdx.x % (uint32_t)a.n_close, job = a.job0 + b;
    const uint32_t pair = job >> a.n_held, hbits = job & ((1u << a.n_held) - 1u);
    const sweep::HeldRep rep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W};
    const sweep::Op<sweep::NarrowOps> op(ops, close_op[ci]);
    const uint32_t pairs = op.w[2], cq = rep(op.w, op.w[3]);
    const double *slice = fwd + (((size_t)b * (size_t)a.n_close + ci) << a.width);
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    for (uint32_t f = lane; f < (1u << op.top); f += marginal::kFoldLanes) {       // top <= width: within the slice
        if (f & ~op.mask) continue;
        const uint32_t idx = marginal_idx(cq, pairs, f);
        const double d = slice[f];
        if (idx == 0u) v0 = v0 + d;
        else if (idx == 1u) v1 = v1 + d;
        else if (idx == 2u) v2 = v2 + d;
        else v3 = v3 + d;
    }
#pragma unroll
    for (int m = (int)marginal::kFoldLanes / 2; m >= 1; m >>= 1) {
        v0 = v0 + __shfl_xor(v0, m, (int)marginal::kFoldLanes);
        v1 = v1 + __shfl_xor(v1, m, (int)marginal::kFoldLanes);
        v2 = v2 + __shfl_xor(v2, m, (int)marginal::kFoldLanes);
        v3 = v3 + __shfl_xor(v3, m, (int)marginal::kFoldLanes);
    }
    if (lane == 0) {
        double *out = Mh + ((size_t)job * (size_t)a.n_close + ci) * 4u;
        out[0] = v0; out[1] = v1; out[2] = v2; out[3] = v3;
    }
}

__global__ __launch_bounds__(sweep::kThreads) void k_class_marginal_combine(const MarginalArgs a, const uint32_t *__restrict__ reps, const int32_t *__restrict__ close_of, double *Mh,
                                                                            const double *__restrict__ z, double *__restrict__ out)
{
    const uint32_t per = (uint32_t)a.n_close * 4u;
    double *mine = Mh + ((size_t)blockIdx.x << a.n_held) * per;
    for (int j = 0; j < a.n_held; ++j) {
        const uint32_t items = (1u << (a.n_held - 1 - j)) * per;
        for (uint32_t i = threadIdx.x; i < items; i += sweep::kThreads) {
            const uint32_t h = (i / per) << (j + 1), e = i % per;
            mine[(size_t)h * per + e] = mine[(size_t)h * per + e] + mine[(size_t)(h | (1u << j)) * per + e];
        }
        __syncthreads();                                      // (the next bit reads what other lanes of this workgroup wrote)
    }
    const uint32_t *rep = reps + (size_t)blockIdx.x * (size_t)a.W;
    double *row = out + (size_t)blockIdx.x * (size_t)a.nq * 4u;
    for (uint32_t i = threadIdx.x; i < (uint32_t)a.nq * 4u; i += sweep::kThreads) {
        const uint32_t q = i >> 2, pauli = i & 3u;
        const int32_t ci = close_of[q];
        if (ci >= 0 && ci < a.n_close) row[i] = mine[(uint32_t)ci * 4u + sweep::pauli_to_xz(pauli)] * a.scale;
        else row[i] = pauli == ((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u) ? z[blockIdx.x] : 0.0;
    }
}

hipError_t class_marginal_allow_lds(int width, int site)
{
    static LdsOptIn fwd, fwd_site, bwd, bwd_site;
    if (site) {
        if (hipError_t e = cut_allow_lds(reinterpret_cast<const void *>(k_class_marginal_fwd_site), fwd_site, width)) return e;
        return cut_allow_lds(reinterpret_cast<const void *>(k_class_marginal_bwd_site), bwd_site, width);
    }
    if (hipError_t e = cut_allow_lds(reinterpret_cast<const void *>(k_class_marginal_fwd), fwd, width)) return e;
    return cut_allow_lds(reinterpret_cast<const void *>(k_class_marginal_bwd), bwd, width);
}

// what every launch here asks: a plan the sweep kernels take, and jobs [job0, job0 + jobs) within the group's and within the workspace
static bool marginal_args_ok(const MarginalArgs &a)
{
    if (!sweep::cut_args_ok(a.S, a.ncls, a.width, a.W, a.n_ops, a.n_held) || a.S < 1u || a.n_close < 1 || a.n_close > a.n_ops || a.nq < 1 || a.nq > 16 * a.W) return false;
    const uint64_t all = ((uint64_t)a.S * (uint64_t)a.ncls) << a.n_held;
    if (a.jobs < 1u || a.jobs > sweep::kCutGridMax || (uint64_t)a.job0 + a.jobs > all) return false;
    const uint64_t bytes = (uint64_t)a.jobs * marginal::marginal_entries_per_job(a.n_close, a.width) * sizeof(double);
    return bytes <= marginal::kMarginalWorkspaceBytes;
}

static bool marginal_site_ok(const MarginalArgs &a, const double *wq) { return !wq || ((reinterpret_cast<uintptr_t>(wq) & 31u) == 0 && (a.per_syndrome == 0 || a.per_syndrome == 1)); }

hipError_t launch_marginal_forward(const MarginalArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *fwd, double *P,
                                   hipStream_t stream)
{
    if (!marginal_args_ok(a) || !marginal_site_ok(a, wq) || !ops || !reps || !fwd || !P || (a.n_held > 0 && !held)) return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_marginal_allow_lds(a.width, wq != nullptr)) return e;
    const dim3 grid(a.jobs), block(sweep::cut_threads(a.width));
    if (wq) hipLaunchKernelGGL(k_class_marginal_fwd_site, grid, block, carve.bytes, stream, a, ops, held, reps, wq, fwd, P);
    else hipLaunchKernelGGL(k_class_marginal_fwd, grid, block, carve.bytes, stream, a, ops, held, reps, fwd, P);
    return hipGetLastError();
}

hipError_t launch_marginal_backward(const MarginalArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *fwd, hipStream_t stream)
{
    if (!marginal_args_ok(a) || !marginal_site_ok(a, wq) || !ops || !reps || !fwd || (a.n_held > 0 && !held)) return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_marginal_allow_lds(a.width, wq != nullptr)) return e;
    const dim3 grid(a.jobs), block(sweep::cut_threads(a.width));
    if (wq) hipLaunchKernelGGL(k_class_marginal_bwd_site, grid, block, carve.bytes, stream, a, ops, held, reps, wq, fwd);
    else hipLaunchKernelGGL(k_class_marginal_bwd, grid, block, carve.bytes, stream, a, ops, held, reps, fwd);
    return hipGetLastError();
}

hipError_t launch_marginal_fold(const MarginalArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *close_op, const double *fwd, double *Mh,
                                hipStream_t stream)
{
    if (!marginal_args_ok(a) || !ops || !reps || !close_op || !fwd || !Mh || (a.n_held > 0 && !held)) return hipErrorInvalidValue;
    const uint64_t slices = (uint64_t)a.jobs * (uint64_t)a.n_close;
    if (slices > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_class_marginal_fold, dim3((uint32_t)slices), dim3(marginal::kFoldLanes), 0, stream, a, ops, held, reps, close_op, fwd, Mh);
    return hipGetLastError();
}

hipError_t launch_marginal_combine(const MarginalArgs &a, const uint32_t *reps, const int32_t *close_of, double *Mh, const double *z, double *out, hipStream_t stream)
{
    if (!sweep::cut_args_ok(a.S, a.ncls, a.width, a.W, a.n_ops, a.n_held) || a.S < 1u || a.n_close < 1 || a.nq < 1 || a.nq > 16 * a.W || !reps || !close_of || !Mh || !z || !out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_class_marginal_combine, dim3(a.S * (uint32_t)a.ncls), dim3(sweep::kThreads), 0, stream, a, reps, close_of, Mh, z, out);
    return hipGetLastError();
}

}  // namespace qecmc
