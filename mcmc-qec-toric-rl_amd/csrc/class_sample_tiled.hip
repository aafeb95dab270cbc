// qecmc_class_sample_tiled, qecmc_class_sample_tiled_site: the exact chain sampler of class_sample_tiled.hpp.  The partials are k_class_sweep_tiled's /
// _tiled_site's (class_sweep_tiled.hip, class_sweep_site.hip), unchanged and left unfolded, the pick is k_class_sample_pick (class_sample.hip); the
// three kernels here run after them on the same stream.  Stream order is the only synchronisation: no atomics, no flags, no scratch, no static LDS,
// no inline assembly.
//
// k_class_sample_tiled_record, k_class_sample_tiled_record_site: the grid (live tiles, jobs of the pass), the block (tiled_threads), the dynamic LDS
// (one tile, 64 KiB at most: within the default limit, no attribute) and the gather / write-back of k_class_sweep_tiled; job blockIdx.y sweeps pair
// job_pair[job] under hbits = job_h[job].  The body is the CLOSE and INTRO passes of class_sweep_ops.hpp and a FORGET that reads off and on from LDS,
// forms s = off + on, stores (on, s) with one 16-byte vector store per lane and puts s back: the very double the FORGET leaves in A[f].  The site form
// differs in the factor source alone (SiteFour for UniformFour).  The last segment stores nothing: the partials are the sweep's.  Dirty HBM, dirty
// LDS and a dirty record are allowed: the walk reads only pairs of live f, which these kernels wrote.
//
// k_class_sample_tiled_walk: launched after the last record segment of the pass, so no kernel reads what it wrote itself.  Each lane owns one sample:
// its f, its Philox draws (one block serves two FORGETs; the block changes under wave-uniform control flow, fi being the same in every lane) and its
// chain, W words in a lane-private column of the dynamic LDS window (256 W bytes, 7 KiB at most; 28 words in registers next to a Philox block pass 64
// VGPRs).  A FORGET touches the words its generator is not 0 in, four at most, under wave-uniform control flow.  The wide ops, the tile table and the
// forget words are wave-uniform scalar loads; the record pair is one 16-byte load per lane, found from the lane's global f through forget_tile.
//
// The unit is built with the tiled sweep's flags (the Makefile's -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero line): s is formed
// by the add the sweep's FORGET makes, and no multiply here feeds an add -- every product is stored or compared.
#include "class_sample_tiled.hpp"
#include "philox.hpp"

namespace qecmc {

constexpr uint32_t kSampleTiledWave = 64;

// One workgroup of a record kernel: live tile blockIdx.x of job a.unit_first + blockIdx.y, sweep::tile_sweep's gather and write-back around the op
// loop with a FORGET that records.  src: the factors of a CLOSE.
template <class Src>
__device__ __forceinline__ void tile_sweep_recorded(double *lds, const SampleTiledArgs &a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                    const uint32_t *__restrict__ reps, uint32_t pair, uint32_t hbits, const uint32_t *__restrict__ forget_tile,
                                                    double *__restrict__ work, double2 *__restrict__ R, const Src &src)
{
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    const uint32_t base = sweep::bits_deposit(blockIdx.x, a.fixed_live), entries = 1u << a.tile_width;
    double *A = work + ((size_t)blockIdx.y << a.state_bits) + base;
    double2 *mine = R + (size_t)blockIdx.y * (size_t)a.pairs_per_job + ((size_t)blockIdx.x << (a.tile_width - 1));
    const uint32_t f0 = sweep::bits_deposit(tid, a.tile), step = sweep::bits_deposit(threads, a.tile);
    if (a.first) {
        if (tid == 0) lds[0] = 1.0;
    } else {
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_in)) lds[l] = A[f];
    }
    __syncthreads();
    const sweep::TileRep rep{sweep::HeldRep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W}, base};
    uint32_t fi = a.forget_first;
    for (uint32_t o = a.op_first; o < a.op_first + a.op_count; ++o) {
        const sweep::Op<sweep::TileOps> op(ops, o);
        if (op.kind == sweep::kClose) sweep::close_pass<sweep::SumProduct>(lds, tid, threads, op, rep, src);
        else if (op.kind == sweep::kIntro) sweep::intro_pass<sweep::SumProduct>(lds, tid, threads, op);
        else {
            const uint32_t n_h = 1u << (op.top - 1u), bit = 1u << op.slot;       // top <= tile_width: h stays within the 2^(tile_width - 1) pairs of the tile
            if (fi < a.n_forget) {                            // (always: the plan counts its FORGETs; a stream that does not cannot leave its record)
                double2 *rows = mine + forget_tile[sample::kTiledForgetWords * fi + 3u];
                for (uint32_t h = tid; h < n_h; h += threads) {
                    const uint32_t f = sweep::insert_zero(h, op.slot);
                    if (f & ~op.mask) continue;
                    const double off = lds[f], on = lds[f | bit], s = sweep::SumProduct::forget(off, on);
                    rows[h] = make_double2(on, s);
                    lds[f] = s;
                }
            }
            ++fi;
        }
        __syncthreads();
    }
    if (!a.last)
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_out)) A[f] = lds[l];
}

__global__ __launch_bounds__(1024) void k_class_sample_tiled_record(const SampleTiledArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                    const uint32_t *__restrict__ reps, const uint32_t *__restrict__ job_pair,
                                                                    const uint32_t *__restrict__ job_h, const uint32_t *__restrict__ forget_tile,
                                                                    double *__restrict__ work, double2 *__restrict__ R)
{
    extern __shared__ double sample_tile_lds[];               // [2^tile_width]
    const uint32_t job = a.unit_first + blockIdx.y, pair = job_pair[job], hbits = job_h ? job_h[job] & ((1u << a.n_held) - 1u) : 0u;
    tile_sweep_recorded(sample_tile_lds, a, ops, held, reps, pair, hbits, forget_tile, work, R, sweep::UniformFour<double>{a.wxz});
}

__global__ __launch_bounds__(1024) void k_class_sample_tiled_record_site(const SampleTiledArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                         const uint32_t *__restrict__ reps, const double *__restrict__ wq,
                                                                         const uint32_t *__restrict__ job_pair, const uint32_t *__restrict__ job_h,
                                                                         const uint32_t *__restrict__ forget_tile, double *__restrict__ work, double2 *__restrict__ R)
{
    extern __shared__ double sample_tile_site_lds[];          // [2^tile_width]
    const uint32_t job = a.unit_first + blockIdx.y, pair = job_pair[job], hbits = job_h ? job_h[job] & ((1u << a.n_held) - 1u) : 0u;
    const double *rows = wq + (size_t)(a.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)a.nq * 4u;
    tile_sweep_recorded(sample_tile_site_lds, a, ops, held, reps, pair, hbits, forget_tile, work, R, sweep::SiteFour<double>{rows});
}

// the bits of v at the positions of m, packed (sweep::bits_extract with the lowest set bit found by __ffs); m is wave-uniform
static __device__ __forceinline__ uint32_t walk_extract(uint32_t v, uint32_t m)
{
    uint32_t out = 0, k = 0;
    for (; m; m &= m - 1u, ++k) out |= ((v >> (uint32_t)(__ffs(m) - 1)) & 1u) << k;
    return out;
}

__global__ __launch_bounds__(kSampleTiledWave) void k_class_sample_tiled_walk(const SampleTiledWalkArgs t, const uint32_t *__restrict__ wide_ops,
                                                                              const uint32_t *__restrict__ held, const uint32_t *__restrict__ reps,
                                                                              const uint32_t *__restrict__ forget_words, const uint32_t *__restrict__ forget_tile,
                                                                              const uint32_t *__restrict__ spair, const uint32_t *__restrict__ sh,
                                                                              const uint32_t *__restrict__ rec_of_pair, const double2 *__restrict__ R,
                                                                              uint8_t *__restrict__ chain_out)
{
    extern __shared__ uint32_t sample_walk_lds[];             // [W][64]: word w of lane l at w * 64 + l -- a lane reads and writes its own column alone
    const uint32_t lane = threadIdx.x, local = blockIdx.x * kSampleTiledWave + lane;
    if (local >= t.count) return;                             // (no barrier and no shuffle below: a lane past the end may leave)
    const uint32_t i = t.first + local, pair = spair[i], hbits = sh[i] & ((1u << t.n_held) - 1u), W = (uint32_t)t.W, half_bits = (uint32_t)t.tile_width - 1u;
    const uint32_t rec = (rec_of_pair ? rec_of_pair[pair] : i) - t.rec_first;
    if (rec >= t.records) return;                             // the record of another pass: that pass walks this sample
    const uint32_t syndrome = t.syndrome0 + pair / (uint32_t)t.ncls, stream = pair % (uint32_t)t.ncls;
    const uint64_t k = (uint64_t)t.k0 + (uint64_t)(i % t.k_chunk);
    const double2 *mine = R + (size_t)rec * (size_t)t.pairs_per_job;
    uint32_t *chain = sample_walk_lds + lane;
    for (uint32_t w = 0; w < W; ++w) {
        uint32_t v = reps[(size_t)pair * W + w];
        for (uint32_t rest = hbits; rest; rest &= rest - 1u) v ^= held[(uint32_t)(__ffs(rest) - 1) * W + w];
        chain[w * kSampleTiledWave] = v;
    }
    uint32_t f = 0, have = 0xFFFFFFFFu;
    u32x4 blk = {0u, 0u, 0u, 0u};
    int fi = t.n_forget;
    for (int o = t.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = wide_ops[sweep::kTiledOpWords * o], kind = w0 & 15u, bit = 1u << ((w0 >> 4) & 31u);
        if (kind == sweep::kIntro) f &= ~bit;
        else if (kind == sweep::kForget && fi > 0) {
            --fi;
            const uint32_t block = 1u + ((uint32_t)fi >> 1);
            if (block != have) {                              // wave-uniform: fi is the same in every lane
                blk = philox_block((k << 16) | (uint64_t)block, sample::kSubSample, syndrome, stream, t.seed_lo, t.seed_hi);
                have = block;
            }
            const double u = (fi & 1) ? sample::u53_of(blk.z, blk.w) : sample::u53_of(blk.x, blk.y);
            const uint32_t *ft = forget_tile + sample::kTiledForgetWords * fi;
            const uint32_t x = walk_extract(f, ft[1]), h = minplus::remove_bit(walk_extract(f, ft[0]), ft[2]);
            const double2 r = mine[(size_t)ft[3] + ((size_t)x << half_bits) + h];      // (on, s)
            const bool take = sample::take_branch(u, r.x, r.y);
            if (take) f |= bit;
            const uint32_t *g = forget_words + (size_t)fi * W;
            for (uint32_t w = 0; w < W; ++w) {
                const uint32_t gw = g[w];                     // wave-uniform: a generator touches four cells, so four words at most are not 0
                if (gw != 0u) chain[w * kSampleTiledWave] ^= take ? gw : 0u;
            }
        }
    }
    uint8_t *out = chain_out + (size_t)i * (size_t)t.nq;
    for (uint32_t q = 0; q < (uint32_t)t.nq; ++q) out[q] = (uint8_t)((chain[(q >> 4) * kSampleTiledWave] >> ((q & 15u) * 2u)) & 3u);
}

// what the kernels index with: a chain word per register, every table with its rows, every FORGET's pairs within a job's record
static bool sample_tiled_plan_ok(const sample::TiledSamplePlan &tsp)
{
    const sweep::TiledPlan &tp = tsp.tiled;
    const sweep::Plan &p = tp.plan;
    if (p.W < 1 || p.W > sample::kTiledMaxWords || p.nq < 1 || p.nq > 16 * p.W || tsp.n_forget < 1 || tsp.pairs_per_job < 1 ||
        tsp.pairs_per_job * sizeof(sample::PairRecord) > sample::kTiledSampleRecordBytesMax || tsp.forget_tile.size() != (size_t)tsp.n_forget * sample::kTiledForgetWords ||
        tsp.forget_words.size() != (size_t)tsp.n_forget * (size_t)p.W || tsp.pair_off.size() != (size_t)tsp.n_forget + 1u || tsp.seg_forget.size() != tp.segments.size() ||
        tp.tile_width < sweep::kTileMinWidth || tp.tile_width > sweep::kTileMaxWidth)
        return false;
    for (size_t s = 0; s < tp.segments.size(); ++s) {
        const uint32_t next = s + 1 < tp.segments.size() ? tsp.seg_forget[s + 1] : (uint32_t)tsp.n_forget;
        for (uint32_t fi = tsp.seg_forget[s]; fi < next; ++fi) {
            if (fi >= (uint32_t)tsp.n_forget) return false;
            const uint32_t *ft = &tsp.forget_tile[(size_t)fi * sample::kTiledForgetWords];
            if (ft[0] != tp.segments[s].tile || ft[1] != (tp.segments[s].live & ~tp.segments[s].tile) || ft[2] >= (uint32_t)tp.tile_width || (uint64_t)ft[3] != tsp.pair_off[fi] ||
                tsp.pair_off[fi] + ((uint64_t)tp.segments[s].n_tiles << (tp.tile_width - 1)) > tsp.pairs_per_job)
                return false;
        }
    }
    return true;
}

hipError_t launch_sample_tiled_record(const sample::TiledSamplePlan &tsp, const double *wxz, int per_syndrome, uint32_t job_first, uint32_t jobs, const uint32_t *dev_ops,
                                      const uint32_t *held, const uint32_t *reps, const double *wq, const uint32_t *job_pair, const uint32_t *job_h, const uint32_t *forget_tile,
                                      double *work, sample::PairRecord *R, hipStream_t stream)
{
    if (jobs == 0) return hipSuccess;
    const sweep::TiledPlan &tp = tsp.tiled;
    const sweep::Plan &p = tp.plan;
    if (!sample_tiled_plan_ok(tsp) || (!wq && !wxz) || (per_syndrome != 0 && per_syndrome != 1) || !job_pair || (tp.n_held > 0 && !job_h) || !forget_tile || !work || !R ||
        (uint64_t)jobs * tsp.pairs_per_job * sizeof(sample::PairRecord) > sample::kTiledSampleRecordBytesMax || (wq && (reinterpret_cast<uintptr_t>(wq) & 31u) != 0))
        return hipErrorInvalidValue;
    SampleTiledArgs a = {};
    if (wxz) for (int i = 0; i < 4; ++i) a.wxz[i] = wxz[i];
    a.ncls = p.ncls; a.nq = p.nq; a.per_syndrome = per_syndrome;
    a.n_forget = (uint32_t)tsp.n_forget; a.pairs_per_job = tsp.pairs_per_job;
    return sweep::tiled_segments(tp, job_first, jobs, a, [&](SampleTiledArgs seg, const sweep::Segment &sg) {
        seg.forget_first = tsp.seg_forget[(size_t)(&sg - tp.segments.data())];
        const dim3 grid(sg.n_tiles, jobs), block(sweep::tiled_threads(tp.tile_width));
        if (wq)
            hipLaunchKernelGGL(k_class_sample_tiled_record_site, grid, block, sweep::lds_carve(tp.tile_width).bytes, stream, seg, dev_ops, held, reps, wq, job_pair, job_h, forget_tile,
                               work, reinterpret_cast<double2 *>(R));
        else
            hipLaunchKernelGGL(k_class_sample_tiled_record, grid, block, sweep::lds_carve(tp.tile_width).bytes, stream, seg, dev_ops, held, reps, job_pair, job_h, forget_tile, work,
                               reinterpret_cast<double2 *>(R));
    });
}

hipError_t launch_sample_tiled_walk(const sample::TiledSamplePlan &tsp, const SampleTiledWalkArgs &t, const uint32_t *wide_ops, const uint32_t *held, const uint32_t *reps,
                                    const uint32_t *forget_words, const uint32_t *forget_tile, const uint32_t *spair, const uint32_t *sh, const uint32_t *rec_of_pair,
                                    const sample::PairRecord *R, uint8_t *chain_out, hipStream_t stream)
{
    if (t.count == 0) return hipSuccess;
    const sweep::TiledPlan &tp = tsp.tiled;
    const sweep::Plan &p = tp.plan;
    if (!sample_tiled_plan_ok(tsp) || t.ncls != p.ncls || t.W != p.W || t.n_held != tp.n_held || t.n_ops != p.n_ops || t.n_forget != tsp.n_forget || t.nq != p.nq ||
        t.tile_width != tp.tile_width || t.pairs_per_job != tsp.pairs_per_job || t.k_chunk < 1 || t.records < 1 || (uint64_t)t.first + t.count > sample::kTiledLaunchSamples ||
        (uint64_t)t.records * tsp.pairs_per_job * sizeof(sample::PairRecord) > sample::kTiledSampleRecordBytesMax || !wide_ops || !forget_words || !forget_tile || !spair || !sh ||
        !R || !chain_out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_class_sample_tiled_walk, dim3((t.count + kSampleTiledWave - 1u) / kSampleTiledWave), dim3(kSampleTiledWave),
                       (size_t)p.W * kSampleTiledWave * sizeof(uint32_t), stream, t, wide_ops, held, reps,
                       forget_words, forget_tile, spair, sh, rec_of_pair, reinterpret_cast<const double2 *>(R), chain_out);
    return hipGetLastError();
}

}  // namespace qecmc
