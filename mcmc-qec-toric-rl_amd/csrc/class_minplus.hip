// qecmc_class_minplus: the (min, +, count) sweep of class_minplus.hpp.
//
// k_class_minplus: grid and block as k_class_sweep_cut (class_sweep_cut.hip) -- workgroup blockIdx.x = ((syndrome * ncls + class) << n_held) + h sweeps
// one representative under one assignment h of the held generators, blockDim = cut_threads(width).  The state vector is uint64_t[2^width] in dynamic
// LDS, one packed (cost, count) entry where the sibling keeps a double; only A[0] = (0, 1) is set up.  The op loop is class_sweep_ops.hpp's in the
// algebra minplus::MinPlus: CLOSE adds the cost of the qubit's Pauli to the upper 16 bits, FORGET is mp_combine.  The four costs are kernel
// arguments.  The packed partial leaves through one vector store, P[blockIdx.x].
//
// k_class_minplus_reduce: workgroup blockIdx.x = syndrome * ncls + class combines its 2^n_held partials in place with mp_combine -- associative and
// commutative, so the order is free; it folds the held bits in ascending order, one barrier per bit --, then unpacks, shifts the count by
// n_gen - rank, reports a saturated count as 0 and writes cost_out and count_out.  It also runs when n_held = 0.  It is launched on the same stream
// after the sweep kernel: stream order is the only synchronisation, there are no flags and no atomics.  Either kernel has a host function of its own
// (launch_class_minplus_sweep, launch_class_minplus_reduce; launch_class_minplus calls both): the traceback (class_minplus_trace.hip) reads the partials
// between the two.
//
// A state vector beyond 64 KiB (width 14) needs the dynamic-LDS limit of k_class_minplus raised (cut_allow_lds, class_sweep_cut.hpp).
#include "class_minplus.hpp"

namespace qecmc {

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_minplus(const MinplusArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                   const uint32_t *__restrict__ reps, uint64_t *__restrict__ P)
{
    extern __shared__ uint64_t minplus_lds[];                 // [2^width]
    const uint32_t tid = threadIdx.x, pair = blockIdx.x >> a.n_held, hbits = blockIdx.x & ((1u << a.n_held) - 1u);
    if (tid == 0) minplus_lds[0] = 1ull;                      // (0, 1)
    __syncthreads();
    sweep::op_loop<sweep::NarrowOps, minplus::MinPlus>(minplus_lds, ops, 0u, (uint32_t)a.n_ops, tid, blockDim.x,
                                                       sweep::HeldRep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W}, sweep::UniformFour<uint32_t>{a.cxz});
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

hipError_t class_minplus_allow_lds(int width)
{
    static LdsOptIn opt;
    return cut_allow_lds(reinterpret_cast<const void *>(k_class_minplus), opt, width);
}

static bool minplus_args_ok(const MinplusArgs &a)
{
    return sweep::cut_args_ok(a.S, a.ncls, a.width, a.W, a.n_ops, a.n_held) && a.shift >= 0 && a.shift < minplus::kCountBits;
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
    // (what the reduce reads, as launch_class_sweep_reduce asks it: the tiled route's partials come from plans wider than an LDS state vector)
    if ((a.ncls != 4 && a.ncls != 16) || a.n_held < 0 || a.n_held > sweep::kMaxHeld || a.S > sweep::cut_launch_group(a.S, a.ncls, a.n_held) || a.shift < 0 ||
        a.shift >= minplus::kCountBits)
        return hipErrorInvalidValue;
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
