// qecmc_class_minplus_tiled_chains, qecmc_class_minplus_tiled_chains_site: the traceback of class_minplus_tiled_trace.hpp.  The partials, the pick and
// the reduce are the shipped kernels', unchanged; the three kernels here run after them on the same stream.  Stream order is the only
// synchronisation: no atomics, no flags, no scratch, no static LDS, no inline assembly.
//
// The unit is built with the Makefile's default flags: the kernels are integer throughout and want no floating-point flag.
//
// k_class_minplus_tiled_trace, k_class_minplus_tiled_trace_site: the grid (live tiles, pairs of the pass), the block (tiled_threads), the dynamic LDS
// (one tile, 64 KiB at most: within the default limit, no attribute) and the gather / write-back of k_class_minplus_tiled(_site); hbits = pick[pair],
// one unit per pair; the body is minplus::tile_sweep_traced.  The site kernel reads the cost word of a CLOSE's qubit through one wave-uniform scalar
// load, the syndrome from the block index alone.
//
// k_minplus_tiled_walk: one wave per pair, launched after the last trace segment of the pass.  f, fi and the op words are the same in every lane;
// lane w < W carries chain word w; at the end the lanes unpack the words to uint8[nq] through shuffles and vector stores, as k_minplus_walk does.
#include "class_minplus_tiled_trace.hpp"

namespace qecmc {

constexpr int kTiledTraceWave = (int)minplus::kTraceWave;

__global__ __launch_bounds__(1024) void k_class_minplus_tiled_trace(const MinplusTiledTraceArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                    const uint32_t *__restrict__ reps, const uint32_t *__restrict__ pick,
                                                                    const uint32_t *__restrict__ forget_tile, uint64_t *__restrict__ work, uint64_t *__restrict__ D)
{
    extern __shared__ uint64_t minplus_tile_trace_lds[];      // [2^tile_width]
    minplus::tile_sweep_traced(minplus_tile_trace_lds, a, ops, held, reps, pick, forget_tile, work, D, sweep::UniformFour<uint32_t>{a.cxz});
}

__global__ __launch_bounds__(1024) void k_class_minplus_tiled_trace_site(const MinplusTiledTraceArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                         const uint32_t *__restrict__ reps, const uint32_t *__restrict__ cw,
                                                                         const uint32_t *__restrict__ pick, const uint32_t *__restrict__ forget_tile,
                                                                         uint64_t *__restrict__ work, uint64_t *__restrict__ D)
{
    extern __shared__ uint64_t minplus_tile_trace_site_lds[]; // [2^tile_width]
    const uint32_t pair = a.unit_first + blockIdx.y;
    const uint32_t *row = cw + (size_t)(a.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)a.nq;
    minplus::tile_sweep_traced(minplus_tile_trace_site_lds, a, ops, held, reps, pick, forget_tile, work, D, minplus::SiteCosts{row});
}

// the bits of v at the positions of m, packed (sweep::bits_extract with the lowest set bit found by __ffs)
static __device__ __forceinline__ uint32_t walk_extract(uint32_t v, uint32_t m)
{
    uint32_t out = 0, k = 0;
    for (; m; m &= m - 1u, ++k) out |= ((v >> (uint32_t)(__ffs(m) - 1)) & 1u) << k;
    return out;
}

__global__ __launch_bounds__(kTiledTraceWave) void k_minplus_tiled_walk(const MinplusTiledWalkArgs t, const uint32_t *__restrict__ wide_ops, const uint32_t *__restrict__ held,
                                                                        const uint32_t *__restrict__ reps, const uint32_t *__restrict__ forget_words,
                                                                        const uint32_t *__restrict__ forget_tile, const uint32_t *__restrict__ pick,
                                                                        const uint64_t *__restrict__ D, uint8_t *__restrict__ chain_out)
{
    const uint32_t lane = threadIdx.x, pair = t.pair_first + blockIdx.x, hbits = pick[pair] & ((1u << t.n_held) - 1u);
    const uint64_t *mine = D + (size_t)blockIdx.x * (size_t)t.words_per_pair;
    uint32_t chain = 0;
    if (lane < (uint32_t)t.W) {
        chain = reps[(size_t)pair * (size_t)t.W + lane];
        for (uint32_t rest = hbits; rest; rest &= rest - 1u) chain ^= held[(uint32_t)(__ffs(rest) - 1) * (uint32_t)t.W + lane];
    }
    uint32_t f = 0;
    int fi = t.n_forget;
    for (int o = t.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = wide_ops[sweep::kTiledOpWords * o], kind = w0 & 15u, bit = 1u << ((w0 >> 4) & 31u);
        if (kind == sweep::kIntro) f &= ~bit;
        else if (kind == sweep::kForget && fi > 0) {
            --fi;
            const uint32_t *ft = forget_tile + minplus::kForgetTileWords * fi;
            const uint32_t x = walk_extract(f, ft[1]), h = minplus::remove_bit(walk_extract(f, ft[0]), ft[2]);
            if ((mine[(size_t)ft[3] + (size_t)x * (size_t)t.words_per_tile + (h >> 6)] >> (h & 63u)) & 1ull) {
                f |= bit;
                if (lane < (uint32_t)t.W) chain ^= forget_words[(size_t)fi * (size_t)t.W + lane];
            }
        }
    }
    uint8_t *out = chain_out + (size_t)pair * (size_t)t.nq;
    for (uint32_t q0 = 0; q0 < (uint32_t)t.nq; q0 += kTiledTraceWave) {           // whole waves: every lane takes part in the shuffle
        const uint32_t q = q0 + lane;
        const uint32_t word = (uint32_t)__shfl((int)chain, (int)((q >> 4) & (kTiledTraceWave - 1u)), kTiledTraceWave);
        if (q < (uint32_t)t.nq) out[q] = (uint8_t)((word >> ((q & 15u) * 2u)) & 3u);
    }
}

hipError_t launch_minplus_tiled_trace(const minplus::TiledTracePlan &ttp, const uint32_t *cxz, int per_syndrome, uint32_t pair_first, uint32_t pairs, const uint32_t *dev_ops,
                                      const uint32_t *wide_ops, const uint32_t *held, const uint32_t *reps, const uint32_t *cw, const uint32_t *pick, const uint32_t *forget_tile,
                                      const uint32_t *forget_words, uint64_t *work, uint64_t *D, uint8_t *chain_out, hipStream_t stream)
{
    if (pairs == 0) return hipSuccess;
    const sweep::TiledPlan &tp = ttp.tiled;
    const sweep::Plan &p = tp.plan;
    // what the kernels index with: the walk keeps a chain word per lane, the decision rows of a pass stay within the block, every table has its rows
    if (p.W < 1 || p.W > kTiledTraceWave || p.nq < 1 || p.nq > 16 * p.W || ttp.n_forget < 1 || ttp.words_per_pair < 1 || ttp.words_per_pair > 0xFFFFFFFFull ||
        ttp.words_per_tile != minplus::tiled_trace_words_per_tile(tp.tile_width) || (uint64_t)pairs * ttp.words_per_pair * 8ull > minplus::kTiledTraceWorkspaceBytes ||
        ttp.forget_tile.size() != (size_t)ttp.n_forget * minplus::kForgetTileWords || ttp.forget_words.size() != (size_t)ttp.n_forget * (size_t)p.W ||
        ttp.seg_forget.size() != tp.segments.size() || (!cw && !cxz) || (per_syndrome != 0 && per_syndrome != 1))
        return hipErrorInvalidValue;
    for (size_t s = 0; s < tp.segments.size(); ++s) {                           // every FORGET's words lie within a pair's row
        const uint32_t next = s + 1 < tp.segments.size() ? ttp.seg_forget[s + 1] : (uint32_t)ttp.n_forget;
        for (uint32_t fi = ttp.seg_forget[s]; fi < next; ++fi) {
            const uint32_t *ft = &ttp.forget_tile[(size_t)fi * minplus::kForgetTileWords];
            if (fi >= (uint32_t)ttp.n_forget || ft[0] != tp.segments[s].tile || ft[2] >= (uint32_t)tp.tile_width ||
                (uint64_t)ft[3] + (uint64_t)tp.segments[s].n_tiles * (uint64_t)ttp.words_per_tile > ttp.words_per_pair)
                return hipErrorInvalidValue;
        }
    }
    MinplusTiledTraceArgs a = {};
    if (cxz) for (int i = 0; i < 4; ++i) a.cxz[i] = cxz[i];
    a.ncls = p.ncls; a.nq = p.nq; a.per_syndrome = per_syndrome;
    a.n_forget = (uint32_t)ttp.n_forget; a.words_per_tile = (uint32_t)ttp.words_per_tile; a.words_per_pair = (uint32_t)ttp.words_per_pair;
    const hipError_t e = sweep::tiled_segments(tp, pair_first, pairs, a, [&](MinplusTiledTraceArgs seg, const sweep::Segment &sg) {
        seg.forget_first = ttp.seg_forget[(size_t)(&sg - tp.segments.data())];
        const dim3 grid(sg.n_tiles, pairs), block(sweep::tiled_threads(tp.tile_width));
        if (cw)
            hipLaunchKernelGGL(k_class_minplus_tiled_trace_site, grid, block, sweep::lds_carve(tp.tile_width).bytes, stream, seg, dev_ops, held, reps, cw, pick, forget_tile, work, D);
        else
            hipLaunchKernelGGL(k_class_minplus_tiled_trace, grid, block, sweep::lds_carve(tp.tile_width).bytes, stream, seg, dev_ops, held, reps, pick, forget_tile, work, D);
    });
    if (e != hipSuccess) return e;
    MinplusTiledWalkArgs t = {};
    t.pair_first = pair_first; t.pairs = pairs; t.W = p.W; t.n_held = tp.n_held; t.n_ops = p.n_ops; t.n_forget = ttp.n_forget; t.nq = p.nq;
    t.words_per_tile = (uint32_t)ttp.words_per_tile; t.words_per_pair = (uint32_t)ttp.words_per_pair;
    hipLaunchKernelGGL(k_minplus_tiled_walk, dim3(pairs), dim3(kTiledTraceWave), 0, stream, t, wide_ops, held, reps, forget_words, forget_tile, pick, D, chain_out);
    return hipGetLastError();
}

}  // namespace qecmc
