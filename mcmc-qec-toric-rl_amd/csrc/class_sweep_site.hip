// qecmc_class_sweep_site, _cut_site, _tiled_site: the three sweeps under a weight per (syndrome, qubit) (class_sweep_site.hpp).
//
// Each kernel is its sibling's -- k_class_sweep (class_sweep.hip), k_class_sweep_cut (class_sweep_cut.hip), k_class_sweep_tiled
// (class_sweep_tiled.hip) -- op for op, entry for entry and barrier for barrier; those comments hold here.  The one difference is in CLOSE: the four
// weights are not kernel arguments but the 32 bytes of the table wq at row (per_syndrome ? syndrome : 0) * nq + q, in (x, z) order.  The syndrome
// comes from the block index alone -- blockIdx.y; (blockIdx.x >> n_held) / ncls; (unit >> n_held) / ncls -- and q from the plan, so the address is
// wave-uniform: the four doubles arrive by one scalar load per CLOSE, next to the scalar loads of the op's words, and no lane carries the table.  The
// two selects and the single multiply per entry follow as in the sibling; values leave through vector stores.  The cut and the tiled route sum their
// partials with k_class_sweep_reduce (class_sweep_cut.hip), on the same stream.
//
// The unit is built without floating-point contraction, without fast-math and without flush-to-zero, as class_sweep_tiled.hip.
#include "class_sweep_site.hpp"

#include <mutex>

namespace qecmc {

__global__ __launch_bounds__(sweep::kThreads) void k_class_sweep_site(const SweepSiteArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ reps,
                                                                      const double *__restrict__ wq, double *__restrict__ z)
{
    extern __shared__ double sweep_site_lds[];                // [2^width]
    const uint32_t tid = threadIdx.x, pair = blockIdx.y * (uint32_t)a.ncls + blockIdx.x;
    const uint32_t *rep = reps + (size_t)pair * (size_t)a.W;
    const double *rows = wq + (size_t)(a.per_syndrome ? blockIdx.y : 0u) * (size_t)a.nq * 4u;
    if (tid == 0) sweep_site_lds[0] = 1.0;
    __syncthreads();
    for (int o = 0; o < a.n_ops; ++o) {
        const uint32_t w0 = ops[4 * o], mask = ops[4 * o + 1];
        const uint32_t kind = w0 & 15u, slot = (w0 >> 4) & 15u, top = (w0 >> 12) & 31u, bit = 1u << slot;
        if (kind == sweep::kClose) {
            const uint32_t pairs = ops[4 * o + 2], q = ops[4 * o + 3];
            const uint32_t cq = sweep::pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
            const double *w = rows + (size_t)q * 4u;
            const double w00 = w[0], w01 = w[1], w10 = w[2], w11 = w[3];
            for (uint32_t f = tid; f < (1u << top); f += sweep::kThreads) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                const double lo = (idx & 1u) ? w01 : w00, hi = (idx & 1u) ? w11 : w10;
                sweep_site_lds[f] = sweep_site_lds[f] * ((idx & 2u) ? hi : lo);
            }
        } else {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += sweep::kThreads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                if (kind == sweep::kIntro) sweep_site_lds[f | bit] = sweep_site_lds[f];
                else sweep_site_lds[f] = sweep_site_lds[f] + sweep_site_lds[f | bit];
            }
        }
        __syncthreads();
    }
    if (tid == 0) z[pair] = sweep_site_lds[0] * a.scale;
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_sweep_cut_site(const SweepSiteArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                                const uint32_t *__restrict__ reps, const double *__restrict__ wq, double *__restrict__ P)
{
    extern __shared__ double sweep_cut_site_lds[];            // [2^width]
    const uint32_t tid = threadIdx.x, threads = blockDim.x, pair = blockIdx.x >> a.n_held, hbits = blockIdx.x & ((1u << a.n_held) - 1u);
    const uint32_t *rep = reps + (size_t)pair * (size_t)a.W;
    const double *rows = wq + (size_t)(a.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)a.nq * 4u;
    if (tid == 0) sweep_cut_site_lds[0] = 1.0;
    __syncthreads();
    for (int o = 0; o < a.n_ops; ++o) {
        const uint32_t w0 = ops[4 * o], mask = ops[4 * o + 1];
        const uint32_t kind = w0 & 15u, slot = (w0 >> 4) & 15u, top = (w0 >> 12) & 31u, bit = 1u << slot;
        if (kind == sweep::kClose) {
            const uint32_t pairs = ops[4 * o + 2], q = ops[4 * o + 3];
            uint32_t word = rep[q >> 4];
            for (uint32_t rest = hbits; rest; rest &= rest - 1u) word ^= held[(uint32_t)(__ffs(rest) - 1) * (uint32_t)a.W + (q >> 4)];
            const uint32_t cq = sweep::pauli_to_xz((word >> ((q & 15u) * 2u)) & 3u);
            const double *w = rows + (size_t)q * 4u;
            const double w00 = w[0], w01 = w[1], w10 = w[2], w11 = w[3];
            for (uint32_t f = tid; f < (1u << top); f += threads) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                const double lo = (idx & 1u) ? w01 : w00, hi = (idx & 1u) ? w11 : w10;
                sweep_cut_site_lds[f] = sweep_cut_site_lds[f] * ((idx & 2u) ? hi : lo);
            }
        } else {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += threads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                if (kind == sweep::kIntro) sweep_cut_site_lds[f | bit] = sweep_cut_site_lds[f];
                else sweep_cut_site_lds[f] = sweep_cut_site_lds[f] + sweep_cut_site_lds[f | bit];
            }
        }
        __syncthreads();
    }
    if (tid == 0) P[blockIdx.x] = sweep_cut_site_lds[0];
}

__global__ __launch_bounds__(1024) void k_class_sweep_tiled_site(const SweepTiledSiteArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                 const uint32_t *__restrict__ reps, const double *__restrict__ wq, double *__restrict__ work,
                                                                 double *__restrict__ P)
{
    extern __shared__ double sweep_tile_site_lds[];           // [2^tile_width]
    const uint32_t tid = threadIdx.x, threads = blockDim.x, unit = a.unit_first + blockIdx.y, hbits = unit & ((1u << a.n_held) - 1u);
    const uint32_t base = sweep::bits_deposit(blockIdx.x, a.fixed_live), entries = 1u << a.tile_width;
    const uint32_t *rep = reps + (size_t)(unit >> a.n_held) * (size_t)a.W;
    const double *rows = wq + (size_t)(a.per_syndrome ? (unit >> a.n_held) / (uint32_t)a.ncls : 0u) * (size_t)a.nq * 4u;
    double *A = work + ((size_t)blockIdx.y << a.state_bits) + base;
    const uint32_t f0 = sweep::bits_deposit(tid, a.tile), step = sweep::bits_deposit(threads, a.tile);
    if (a.first) {
        if (tid == 0) sweep_tile_site_lds[0] = 1.0;
    } else {
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_in)) sweep_tile_site_lds[l] = A[f];
    }
    __syncthreads();
    for (uint32_t o = a.op_first; o < a.op_first + a.op_count; ++o) {
        const uint32_t w0 = ops[5 * o], mask = ops[5 * o + 1];
        const uint32_t kind = w0 & 15u, slot = (w0 >> 4) & 15u, top = (w0 >> 8) & 31u, bit = 1u << slot;
        if (kind == sweep::kClose) {
            const uint32_t pairs = ops[5 * o + 2], q = ops[5 * o + 3], fixed = ops[5 * o + 4];
            uint32_t word = rep[q >> 4];
            for (uint32_t rest = hbits; rest; rest &= rest - 1u) word ^= held[(uint32_t)(__ffs(rest) - 1) * (uint32_t)a.W + (q >> 4)];
            uint32_t cq = sweep::pauli_to_xz((word >> ((q & 15u) * 2u)) & 3u);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t pr = (fixed >> (8 * j)) & 0xFFu;
                cq ^= (0u - ((base >> (pr & 31u)) & 1u)) & (pr >> 5);
            }
            const double *w = rows + (size_t)q * 4u;
            const double w00 = w[0], w01 = w[1], w10 = w[2], w11 = w[3];
            for (uint32_t f = tid; f < (1u << top); f += threads) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                const double lo = (idx & 1u) ? w01 : w00, hi = (idx & 1u) ? w11 : w10;
                sweep_tile_site_lds[f] = sweep_tile_site_lds[f] * ((idx & 2u) ? hi : lo);
            }
        } else {
            for (uint32_t h = tid; h < (1u << (top - 1u)); h += threads) {
                const uint32_t f = sweep::insert_zero(h, slot);
                if (f & ~mask) continue;
                if (kind == sweep::kIntro) sweep_tile_site_lds[f | bit] = sweep_tile_site_lds[f];
                else sweep_tile_site_lds[f] = sweep_tile_site_lds[f] + sweep_tile_site_lds[f | bit];
            }
        }
        __syncthreads();
    }
    if (a.last) {
        if (tid == 0) P[unit] = sweep_tile_site_lds[0];
    } else {
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_out)) A[f] = sweep_tile_site_lds[l];
    }
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

// class_sweep_cut_allow_lds()'s rule for k_class_sweep_cut_site: the dynamic-LDS limit raised once per device, hipErrorInvalidValue where refused
hipError_t class_sweep_cut_site_allow_lds(int width)
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
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_class_sweep_cut_site), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sweep::kCutLdsBudget);
        if (e != hipSuccess) (void)hipGetLastError();         // (the refusal is reported by value; it is not left behind as the thread's last error)
        state[dev] = e == hipSuccess ? 1 : -1;
    }
    return state[dev] == 1 ? hipSuccess : hipErrorInvalidValue;
}

hipError_t launch_class_sweep_cut_site(const SweepSiteArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, double *P, double *z,
                                       hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    if ((a.ncls != 4 && a.ncls != 16) || !sweep::cut_fits(a.width) || a.W < 1 || a.n_ops < 1 || a.n_held < 0 || a.n_held > sweep::kMaxHeld ||
        a.S > sweep::cut_launch_group(a.S, a.ncls, a.n_held) || !site_table_ok(wq, a.nq, a.per_syndrome))
        return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_sweep_cut_site_allow_lds(a.width)) return e;
    const uint32_t pairs = a.S * (uint32_t)a.ncls;
    hipLaunchKernelGGL(k_class_sweep_cut_site, dim3(pairs << a.n_held), dim3(sweep::cut_threads(a.width)), carve.bytes, stream, a, ops, held, reps, wq, P);
    if (hipError_t e = hipGetLastError()) return e;
    SweepCutArgs ra = {};
    ra.S = a.S; ra.ncls = a.ncls; ra.W = a.W; ra.width = a.width; ra.n_ops = a.n_ops; ra.n_held = a.n_held; ra.scale = a.scale;
    return launch_class_sweep_reduce(ra, P, z, stream);
}

hipError_t launch_class_sweep_tiled_site(const sweep::TiledPlan &tp, int per_syndrome, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                         const uint32_t *reps, const double *wq, double *work, double *P, hipStream_t stream)
{
    if (units == 0) return hipSuccess;
    const sweep::Plan &p = tp.plan;
    if ((p.ncls != 4 && p.ncls != 16) || tp.tile_width < sweep::kTileMinWidth || tp.tile_width > sweep::kTileMaxWidth || tp.state_bits < tp.tile_width ||
        tp.state_bits > sweep::kTiledMaxWidth || p.W < 1 || p.n_ops < 1 || tp.n_held < 0 || tp.n_held > sweep::kMaxHeld || units > sweep::tiled_pass_units(tp.state_bits) ||
        tp.segments.empty() || !site_table_ok(wq, p.nq, per_syndrome))
        return hipErrorInvalidValue;
    SweepTiledSiteArgs a = {};
    a.unit_first = unit_first; a.units = units; a.W = p.W; a.n_held = tp.n_held; a.state_bits = tp.state_bits; a.tile_width = tp.tile_width;
    a.ncls = p.ncls; a.nq = p.nq; a.per_syndrome = per_syndrome;
    for (size_t s = 0; s < tp.segments.size(); ++s) {
        const sweep::Segment &sg = tp.segments[s];
        a.op_first = sg.op_first; a.op_count = sg.op_count; a.tile = sg.tile; a.fixed_live = sg.live & ~sg.tile;
        a.local_in = sweep::bits_extract(sg.live_in, sg.tile); a.local_out = sweep::bits_extract(sg.live_out, sg.tile);
        a.n_tiles = sg.n_tiles; a.first = s == 0; a.last = s + 1 == tp.segments.size();
        if ((int)sweep::popcount32(sg.tile) != tp.tile_width || (sg.tile >> tp.state_bits) != 0u || (sg.live >> tp.state_bits) != 0u ||
            sg.n_tiles != 1u << sweep::popcount32(a.fixed_live) || sg.op_first + sg.op_count > (uint32_t)p.n_ops)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_class_sweep_tiled_site, dim3(sg.n_tiles, units), dim3(sweep::tiled_threads(tp.tile_width)), sweep::lds_carve(tp.tile_width).bytes, stream, a,
                           dev_ops, held, reps, wq, work, P);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace qecmc
