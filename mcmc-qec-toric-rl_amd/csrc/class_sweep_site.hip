// qecmc_class_sweep_site, _cut_site, _tiled_site: the three sweeps under a weight per (syndrome, qubit) (class_sweep_site.hpp).
//
// Each kernel has its sibling's grid, block and write-out -- k_class_sweep (class_sweep.hip), k_class_sweep_cut (class_sweep_cut.hip),
// k_class_sweep_tiled (class_sweep_tiled.hip) -- and the op loop of class_sweep_ops.hpp.  What is theirs is the factor source of a CLOSE: the four
// weights are not kernel arguments but the 32 bytes of the table wq at row (per_syndrome ? syndrome : 0) * nq + q, in (x, z) order.  The syndrome
// comes from the block index alone -- blockIdx.y; (blockIdx.x >> n_held) / ncls; (unit >> n_held) / ncls -- and q from the plan, so the address is
// wave-uniform: the four doubles arrive by one scalar load per CLOSE, next to the scalar loads of the op's words, and no lane carries the table.  The
// cut and the tiled route sum their partials with k_class_sweep_reduce (class_sweep_cut.hip), on the same stream.
//
// The unit is built without floating-point contraction, without fast-math and without flush-to-zero, as class_sweep_tiled.hip.
#include "class_sweep_site.hpp"

namespace qecmc {

__global__ __launch_bounds__(sweep::kThreads) void k_class_sweep_site(const SweepSiteArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ reps,
                                                                      const double *__restrict__ wq, double *__restrict__ z)
{
    extern __shared__ double sweep_site_lds[];                // [2^width]
    const uint32_t tid = threadIdx.x, pair = blockIdx.y * (uint32_t)a.ncls + blockIdx.x;
    const double *rows = wq + (size_t)(a.per_syndrome ? blockIdx.y : 0u) * (size_t)a.nq * 4u;
    if (tid == 0) sweep_site_lds[0] = 1.0;
    __syncthreads();
    sweep::op_loop<sweep::NarrowOps, sweep::SumProduct>(sweep_site_lds, ops, 0u, (uint32_t)a.n_ops, tid, (uint32_t)sweep::kThreads,
                                                        sweep::Rep{reps + (size_t)pair * (size_t)a.W}, sweep::SiteFour<double>{rows});
    if (tid == 0) z[pair] = sweep_site_lds[0] * a.scale;
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_sweep_cut_site(const SweepSiteArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                                const uint32_t *__restrict__ reps, const double *__restrict__ wq, double *__restrict__ P)
{
    extern __shared__ double sweep_cut_site_lds[];            // [2^width]
    const uint32_t tid = threadIdx.x, pair = blockIdx.x >> a.n_held, hbits = blockIdx.x & ((1u << a.n_held) - 1u);
    const double *rows = wq + (size_t)(a.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)a.nq * 4u;
    if (tid == 0) sweep_cut_site_lds[0] = 1.0;
    __syncthreads();
    sweep::op_loop<sweep::NarrowOps, sweep::SumProduct>(sweep_cut_site_lds, ops, 0u, (uint32_t)a.n_ops, tid, blockDim.x,
                                                        sweep::HeldRep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W}, sweep::SiteFour<double>{rows});
    if (tid == 0) P[blockIdx.x] = sweep_cut_site_lds[0];
}

__global__ __launch_bounds__(1024) void k_class_sweep_tiled_site(const SweepTiledSiteArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                 const uint32_t *__restrict__ reps, const double *__restrict__ wq, double *__restrict__ work,
                                                                 double *__restrict__ P)
{
    extern __shared__ double sweep_tile_site_lds[];           // [2^tile_width]
    const uint32_t unit = a.unit_first + blockIdx.y;
    const double *rows = wq + (size_t)(a.per_syndrome ? (unit >> a.n_held) / (uint32_t)a.ncls : 0u) * (size_t)a.nq * 4u;
    sweep::tile_sweep<sweep::SumProduct>(sweep_tile_site_lds, a, ops, held, reps, work, P, sweep::SiteFour<double>{rows});
}

// what every launch asks of the table: a pointer on a 32-byte boundary, a qubit count, a flag
static bool site_table_ok(const double *wq, int nq, int per_syndrome)
{
    return wq && (reinterpret_cast<uintptr_t>(wq) & 31u) == 0 && nq >= 1 && (per_syndrome == 0 || per_syndrome == 1);
}

hipError_t launch_class_sweep_site(const SweepSiteArgs &a, const uint32_t *ops, const uint32_t *reps, const double *wq, double *z, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if ((a.ncls != 4 && a.ncls != 16) || a.width < 1 || a.width > sweep::kMaxWidth || carve.bytes == 0 || carve.bytes > sweep::kLdsBudget || a.W < 1 ||
        a.n_ops < 1 || a.S > sweep::kGroupMax || !site_table_ok(wq, a.nq, a.per_syndrome))
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)a.ncls, a.S), block(sweep::kThreads);
    hipLaunchKernelGGL(k_class_sweep_site, grid, block, carve.bytes, stream, a, ops, reps, wq, z);
    return hipGetLastError();
}

hipError_t class_sweep_cut_site_allow_lds(int width)
{
    static LdsOptIn opt;
    return cut_allow_lds(reinterpret_cast<const void *>(k_class_sweep_cut_site), opt, width);
}

hipError_t launch_class_sweep_cut_site_partials(const SweepSiteArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *P,
                                                hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if (!sweep::cut_args_ok(a.S, a.ncls, a.width, a.W, a.n_ops, a.n_held) || !site_table_ok(wq, a.nq, a.per_syndrome)) return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_sweep_cut_site_allow_lds(a.width)) return e;
    const uint32_t pairs = a.S * (uint32_t)a.ncls;
    hipLaunchKernelGGL(k_class_sweep_cut_site, dim3(pairs << a.n_held), dim3(sweep::cut_threads(a.width)), carve.bytes, stream, a, ops, held, reps, wq, P);
    return hipGetLastError();
}

hipError_t launch_class_sweep_cut_site(const SweepSiteArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *P, double *z,
                                       hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if (hipError_t e = launch_class_sweep_cut_site_partials(a, ops, held, reps, wq, P, stream)) return e;
    SweepCutArgs ra = {};
    ra.S = a.S; ra.ncls = a.ncls; ra.W = a.W; ra.width = a.width; ra.n_ops = a.n_ops; ra.n_held = a.n_held; ra.scale = a.scale;
    return launch_class_sweep_reduce(ra, P, z, stream);
}

hipError_t launch_class_sweep_tiled_site(const sweep::TiledPlan &tp, int per_syndrome, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                         const uint32_t *reps, const double *wq, double *work, double *P, hipStream_t stream)
{
    if (units == 0) return hipSuccess;
    if (!site_table_ok(wq, tp.plan.nq, per_syndrome)) return hipErrorInvalidValue;
    SweepTiledSiteArgs a = {};
    a.ncls = tp.plan.ncls; a.nq = tp.plan.nq; a.per_syndrome = per_syndrome;
    return sweep::tiled_segments(tp, unit_first, units, a, [&](const SweepTiledSiteArgs &seg, const sweep::Segment &sg) {
        hipLaunchKernelGGL(k_class_sweep_tiled_site, dim3(sg.n_tiles, units), dim3(sweep::tiled_threads(tp.tile_width)), sweep::lds_carve(tp.tile_width).bytes, stream, seg,
                           dev_ops, held, reps, wq, work, P);
    });
}

}  // namespace qecmc
