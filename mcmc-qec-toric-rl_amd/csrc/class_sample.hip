// qecmc_class_sample, qecmc_class_sample_site: the exact chain sampler of class_sample.hpp.  The partials are k_class_sweep_cut's / _cut_site's
// (class_sweep_cut.hip, class_sweep_site.hip), unchanged and left unfolded; the four kernels here run after them on the same stream.  Stream order
// is the only synchronisation: no atomics, no flags, no scratch, no static LDS.
//
// k_class_sample_pick: one lane per sample of the launch.  In posterior mode the lane first draws its class from the running sums of z; then, where
// generators are held, it forms the running sums of its pair's partials by sequential adds in ascending h -- the twin's order: every lane is the
// "one lane" of its own sample -- and keeps the lowest h with u * C_last < C_h || C_h == C_last.  pair, h* and class leave through vector stores.
//
// k_class_sample_record, k_class_sample_record_site: the grid is the jobs; block size and dynamic LDS are k_class_sweep_cut's (cut_threads,
// lds_carve).  Job blockIdx.x sweeps pair job_pair[job] under hbits = job_h[job] with the CLOSE and INTRO passes of class_sweep_ops.hpp and a FORGET
// pass that stores (on, s) with one 16-byte vector store per lane before it writes s back: the very double the FORGET leaves in A[f].  The site form
// differs in the factor source alone (SiteFour for UniformFour).  Dirty LDS and a dirty record are allowed: the walk reads only pairs of live f,
// which this kernel wrote.
//
// k_class_sample_walk: launched after the record kernel, so no kernel reads what it wrote itself.  Each lane owns one sample: its f, its Philox
// draws (one block serves two FORGETs; the block changes under wave-uniform control flow, fi being the same in every lane) and its chain, kMaxWords
// statically indexed registers.  The ops and the forget words are wave-uniform scalar loads; the record pair is one 16-byte load per lane.
//
// The unit is built without floating-point contraction, as class_sweep_cut.hip (the Makefile's -ffp-contract=off line); doubles keep their denormals
// on this target whatever the flags, and no multiply here feeds an add: every product is stored or compared.
#include "class_sample.hpp"
#include "philox.hpp"

namespace qecmc {

constexpr uint32_t kSampleWave = 64;

__device__ __forceinline__ double sample_u53(uint64_t k, uint32_t block, uint32_t syndrome, uint32_t stream, const SampleArgs &a)
{
    const u32x4 b = philox_block((k << 16) | (uint64_t)block, sample::kSubSample, syndrome, stream, a.seed_lo, a.seed_hi);
    return sample::u53_of(b.x, b.y);
}

// the lowest index whose running sum passes u * (the last running sum), or has reached it: sequential adds in ascending order
__device__ __forceinline__ uint32_t lowest_running(const double *__restrict__ v, uint32_t n, double u)
{
    double last = v[0];
    for (uint32_t i = 1; i < n; ++i) last = last + v[i];
    const double t = u * last;
    double run = v[0];
    uint32_t i = 0;
    while (!(t < run || run == last) && i + 1u < n) { ++i; run = run + v[i]; }
    return i;
}

__global__ __launch_bounds__(kSampleWave) void k_class_sample_pick(const SampleArgs a, const double *__restrict__ P, const double *__restrict__ z, int32_t *__restrict__ cls,
                                                                   uint32_t *__restrict__ spair, uint32_t *__restrict__ sh)
{
    const uint32_t i = blockIdx.x * kSampleWave + threadIdx.x;
    if (i >= a.n_samples) return;
    const uint32_t group = i / a.k_chunk, ncls = (uint32_t)a.ncls;
    const uint64_t k = (uint64_t)a.k0 + (uint64_t)(i % a.k_chunk);
    uint32_t pair = group;
    if (a.mode) {
        const uint32_t c = lowest_running(z + (size_t)group * ncls, ncls, sample_u53(k, 0u, a.syndrome0 + group, ncls, a));
        cls[i] = (int32_t)c;
        pair = group * ncls + c;
    }
    uint32_t h = 0;
    if (a.n_held > 0) h = lowest_running(P + ((size_t)pair << a.n_held), 1u << a.n_held, sample_u53(k, 0u, a.syndrome0 + pair / ncls, pair % ncls, a));
    spair[i] = pair;
    sh[i] = h;
}

// One workgroup of a record kernel: job blockIdx.x, its pair and hbits from the job table.  src: the factors of a CLOSE.
template <class Src>
__device__ __forceinline__ void record_sweep(double *A, const SampleArgs &a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held, const uint32_t *__restrict__ reps,
                                             uint32_t pair, uint32_t hbits, double2 *__restrict__ R, const Src &src)
{
    const uint32_t tid = threadIdx.x, threads = blockDim.x, half_bits = (uint32_t)a.width - 1u;
    const sweep::HeldRep rep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W};
    double2 *mine = R + ((size_t)blockIdx.x * (size_t)a.n_forget << half_bits);
    int fi = 0;
    if (tid == 0) A[0] = 1.0;
    __syncthreads();
    for (uint32_t o = 0; o < (uint32_t)a.n_ops; ++o) {
        const sweep::Op<sweep::NarrowOps> op(ops, o);
        if (op.kind == sweep::kClose) sweep::close_pass<sweep::SumProduct>(A, tid, threads, op, rep, src);
        else if (op.kind == sweep::kIntro) sweep::intro_pass<sweep::SumProduct>(A, tid, threads, op);
        else {
            const uint32_t n_h = 1u << (op.top - 1u), bit = 1u << op.slot;       // top <= width: h stays within the 2^(width - 1) pairs of FORGET fi
            if (fi < a.n_forget)                              // (always: the plan counts its FORGETs; a stream that does not cannot leave its record)
                for (uint32_t h = tid; h < n_h; h += threads) {
                    const uint32_t f = sweep::insert_zero(h, op.slot);
                    if (f & ~op.mask) continue;
                    const double off = A[f], on = A[f | bit], s = sweep::SumProduct::forget(off, on);
                    mine[((size_t)fi << half_bits) + h] = make_double2(on, s);
                    A[f] = s;
                }
            ++fi;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_sample_record(const SampleArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                         const uint32_t *__restrict__ reps, const uint32_t *__restrict__ job_pair,
                                                                         const uint32_t *__restrict__ job_h, double2 *__restrict__ R)
{
    extern __shared__ double sample_lds[];                    // [2^width]
    const uint32_t pair = job_pair[blockIdx.x], hbits = job_h ? job_h[blockIdx.x] & ((1u << a.n_held) - 1u) : 0u;
    record_sweep(sample_lds, a, ops, held, reps, pair, hbits, R, sweep::UniformFour<double>{a.wxz});
}

__global__ __launch_bounds__(sweep::kCutThreadsMax) void k_class_sample_record_site(const SampleArgs a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                                              const uint32_t *__restrict__ reps, const double *__restrict__ wq,
                                                                              const uint32_t *__restrict__ job_pair, const uint32_t *__restrict__ job_h,
                                                                              double2 *__restrict__ R)
{
    extern __shared__ double sample_site_lds[];               // [2^width]
    const uint32_t pair = job_pair[blockIdx.x], hbits = job_h ? job_h[blockIdx.x] & ((1u << a.n_held) - 1u) : 0u;
    const double *rows = wq + (size_t)(a.per_syndrome ? pair / (uint32_t)a.ncls : 0u) * (size_t)a.nq * 4u;
    record_sweep(sample_site_lds, a, ops, held, reps, pair, hbits, R, sweep::SiteFour<double>{rows});
}

__global__ __launch_bounds__(kSampleWave) void k_class_sample_walk(const SampleArgs a, uint32_t first, uint32_t count, const uint32_t *__restrict__ ops,
                                                                   const uint32_t *__restrict__ held, const uint32_t *__restrict__ reps,
                                                                   const uint32_t *__restrict__ forget_words, const uint32_t *__restrict__ spair,
                                                                   const uint32_t *__restrict__ sh, const uint32_t *__restrict__ rec_of_pair, const double2 *__restrict__ R,
                                                                   uint32_t records, uint8_t *__restrict__ chain_out)
{
    constexpr int MW = sample::kMaxWords;
    const uint32_t local = blockIdx.x * kSampleWave + threadIdx.x;
    if (local >= count) return;                               // (no barrier and no shuffle below: a lane past the end may leave)
    const uint32_t i = first + local, pair = spair[i], hbits = sh[i] & ((1u << a.n_held) - 1u), W = (uint32_t)a.W, half_bits = (uint32_t)a.width - 1u;
    const uint32_t syndrome = a.syndrome0 + pair / (uint32_t)a.ncls, stream = pair % (uint32_t)a.ncls;
    const uint64_t k = (uint64_t)a.k0 + (uint64_t)(i % a.k_chunk);
    const uint32_t rec = rec_of_pair ? rec_of_pair[pair] : local;
    if (rec >= records) return;                               // (never: the host maps every drawn pair to a record of this launch)
    const double2 *mine = R + ((size_t)rec * (size_t)a.n_forget << half_bits);
    uint32_t chain[MW];
#pragma unroll
    for (int w = 0; w < MW; ++w) chain[w] = (uint32_t)w < W ? reps[(size_t)pair * W + (uint32_t)w] : 0u;
    for (uint32_t rest = hbits; rest; rest &= rest - 1u) {
        const uint32_t *g = held + (uint32_t)(__ffs(rest) - 1) * W;
#pragma unroll
        for (int w = 0; w < MW; ++w)
            if ((uint32_t)w < W) chain[w] ^= g[w];
    }
    uint32_t f = 0, have = 0xFFFFFFFFu;
    u32x4 blk = {0u, 0u, 0u, 0u};
    int fi = a.n_forget;
    for (int o = a.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = ops[4 * o], kind = w0 & 15u, slot = (w0 >> 4) & 15u, bit = 1u << slot;
        if (kind == sweep::kIntro) f &= ~bit;
        else if (kind == sweep::kForget && fi > 0) {
            --fi;
            const uint32_t block = 1u + ((uint32_t)fi >> 1);
            if (block != have) {                              // wave-uniform: fi is the same in every lane
                blk = philox_block((k << 16) | (uint64_t)block, sample::kSubSample, syndrome, stream, a.seed_lo, a.seed_hi);
                have = block;
            }
            const double u = (fi & 1) ? sample::u53_of(blk.z, blk.w) : sample::u53_of(blk.x, blk.y);
            const double2 r = mine[((size_t)fi << half_bits) + minplus::remove_bit(f, slot)];      // (on, s); f has bits below width only
            const bool take = u * r.y < r.x || r.x == r.y;
            if (take) f |= bit;
            const uint32_t *g = forget_words + (size_t)fi * W;
#pragma unroll
            for (int w = 0; w < MW; ++w)
                if ((uint32_t)w < W) chain[w] ^= take ? g[w] : 0u;
        }
    }
    uint8_t *out = chain_out + (size_t)i * (size_t)a.nq;
#pragma unroll
    for (int w = 0; w < MW; ++w)
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (w * 16 + j < a.nq) out[w * 16 + j] = (uint8_t)((chain[w] >> (2 * j)) & 3u);
}

hipError_t class_sample_allow_lds(int width, int site)
{
    static LdsOptIn uniform, table;
    return site ? cut_allow_lds(reinterpret_cast<const void *>(k_class_sample_record_site), table, width)
                : cut_allow_lds(reinterpret_cast<const void *>(k_class_sample_record), uniform, width);
}

static bool sample_args_ok(const SampleArgs &a)
{
    return (a.ncls == 4 || a.ncls == 16) && sweep::cut_fits(a.width) && a.W >= 1 && a.W <= sample::kMaxWords && a.n_ops >= 1 && a.n_held >= 0 && a.n_held <= sweep::kMaxHeld &&
           a.n_forget >= 1 && a.nq >= 1 && a.nq <= 16 * a.W && (a.mode == 0 || a.mode == 1) && a.k_chunk >= 1 && a.n_samples >= 1 && a.n_samples % a.k_chunk == 0 &&
           a.n_samples <= sample::kLaunchSamples;
}

// what k_class_sample_pick reads of its arguments, and nothing else: the counts, the mode and the holds (the draws' address is taken as it is).  The
// tiled route (class_sample_tiled.hpp) launches the pick on plans whose width and chain words are not a cut plan's
static bool pick_args_ok(const SampleArgs &a)
{
    return (a.ncls == 4 || a.ncls == 16) && a.n_held >= 0 && a.n_held <= sweep::kMaxHeld && (a.mode == 0 || a.mode == 1) && a.k_chunk >= 1 && a.n_samples >= 1 &&
           a.n_samples % a.k_chunk == 0 && a.n_samples <= sample::kLaunchSamples;
}

hipError_t launch_sample_pick(const SampleArgs &a, const double *P, const double *z, int32_t *cls, uint32_t *spair, uint32_t *sh, hipStream_t stream)
{
    if (!pick_args_ok(a) || !z || !spair || !sh || (a.mode && !cls) || (a.n_held > 0 && !P)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_class_sample_pick, dim3((a.n_samples + kSampleWave - 1u) / kSampleWave), dim3(kSampleWave), 0, stream, a, P, z, cls, spair, sh);
    return hipGetLastError();
}

hipError_t launch_sample_record(const SampleArgs &a, uint32_t jobs, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, const uint32_t *job_pair,
                                const uint32_t *job_h, sample::PairRecord *R, hipStream_t stream)
{
    if (jobs == 0) return hipSuccess;
    if (!sample_args_ok(a) || !job_pair || !R || (a.n_held > 0 && !job_h) || jobs > sweep::kCutGridMax ||
        (uint64_t)jobs * sample::sample_pairs_per_job(a.n_forget, a.width) * sizeof(sample::PairRecord) > sample::kSampleWorkspaceBytes)
        return hipErrorInvalidValue;
    if (wq && ((reinterpret_cast<uintptr_t>(wq) & 31u) != 0 || (a.per_syndrome != 0 && a.per_syndrome != 1))) return hipErrorInvalidValue;
    const sweep::Carve carve = sweep::lds_carve(a.width);
    if (hipError_t e = class_sample_allow_lds(a.width, wq != nullptr)) return e;
    const dim3 grid(jobs), block(sweep::cut_threads(a.width));
    if (wq) hipLaunchKernelGGL(k_class_sample_record_site, grid, block, carve.bytes, stream, a, ops, held, reps, wq, job_pair, job_h, reinterpret_cast<double2 *>(R));
    else hipLaunchKernelGGL(k_class_sample_record, grid, block, carve.bytes, stream, a, ops, held, reps, job_pair, job_h, reinterpret_cast<double2 *>(R));
    return hipGetLastError();
}

hipError_t launch_sample_walk(const SampleArgs &a, uint32_t first, uint32_t count, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *forget_words,
                              const uint32_t *spair, const uint32_t *sh, const uint32_t *rec_of_pair, const sample::PairRecord *R, uint32_t records, uint8_t *chain_out,
                              hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (!sample_args_ok(a) || (uint64_t)first + count > a.n_samples || !spair || !sh || !R || !chain_out || !forget_words || records == 0 ||
        (uint64_t)records * sample::sample_pairs_per_job(a.n_forget, a.width) * sizeof(sample::PairRecord) > sample::kSampleWorkspaceBytes || (!rec_of_pair && records < count))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_class_sample_walk, dim3((count + kSampleWave - 1u) / kSampleWave), dim3(kSampleWave), 0, stream, a, first, count, ops, held, reps, forget_words, spair, sh,
                       rec_of_pair, reinterpret_cast<const double2 *>(R), records, chain_out);
    return hipGetLastError();
}

}  // namespace qecmc
