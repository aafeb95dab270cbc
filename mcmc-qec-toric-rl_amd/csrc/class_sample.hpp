// Exact chains of every class: the sum-product cut sweep of class_sweep_cut.hpp run forward with a record and walked back with draws -- forward
// filtering, backward sampling.  Where class_minplus_trace.hpp asks at every FORGET "which branch is cheaper", this asks "which branch, with
// probability on / (off + on)"; the walk is the same.  A chain of class c is drawn with probability w(chain) / Z_c.
//
// THE RULE, for syndrome s (global index first_syndrome + s), class c, sample k, with the cut plan cp of (code, L, lds_width), the class
// representative rep_c and the factors w (four per call, or a site table).  A uniform is
//     u53(block, j) = (double)(((uint64)word[2j] << 21) | (word[2j + 1] >> 11)) * 2^-53
// of philox_block(k << 16 | block, kSubSample, first_syndrome + s, stream, seed).
//     1. PARTIALS   P[h] for every assignment h of the held generators, as sweep_cut_host forms them; Z_c = cut_reduce of them: qecmc_class_sweep_cut's bits.
//     2. PICK       (n_held > 0 only; else h* = 0 and no draw is spent)  C_0 = P[0], C_h = C_(h-1) + P[h], sequential adds in ascending h;
//                   u = u53(0, 0) on stream c; h* = the lowest h with u * C_last < C_h || C_h == C_last.  One multiply, two compares, no division anywhere.
//     3. RECORD     the op loop under h*; at FORGET number fi (its ordinal in the stream), for every live f with the slot bit clear the pair
//                       (on, s) = (A[f | bit], A[f] + A[f | bit])        -- s is the very double the FORGET leaves in A[f] --
//                   is kept at (fi, h), h = remove_bit(f, slot): 16 bytes, record[fi * 2^(width - 1) + h].  Dead f keep nothing and are never read.
//     4. WALK       f = 0, chain = cut_representative(cp, rep_c, h*); through the ops in reverse: FORGET: (on, s) at (fi, remove_bit(f, slot)),
//                   u = u53(1 + (fi >> 1), fi & 1) on stream c, the generator is taken iff u * s < on || on == s: f |= bit, chain ^= forget_words[fi];
//                   INTRO: f &= ~bit; CLOSE: nothing.  The walk ends at f == 0.
//     5. RESULT     the chain as bytes uint8[nq]; a cell no generator touches keeps the representative's byte.
// POSTERIOR MODE draws the class first: running sums of Z_c in ascending c, u = u53(0, 0) on stream ncls -- which no class owns --, the class is
// the lowest c with u * Z_total < (running sum) || (running sum) == Z_total; sample (s, k) of the posterior is then sample (s, cls[s, k], k) of the
// every-class mode.
//
// A sample depends on (seed, first_syndrome + s, c, k, plan, representative, weights) alone: not on N, K, the launch grouping or the other samples.
// Every taken branch has probability on / s up to the 2^-53 grain of u and one rounding.  SUPPORT holds at every range by construction, not by a
// floor: the walk starts at a partial > 0 (a pick never lands on an entry of 0: its running sum is its predecessor's, which would have been picked) and
// s > 0 at every FORGET on its path, so on == 0 is never taken (u * s < 0 is false, and on == s would make s 0), and a branch is declined only where
// on != s, that is off != 0.  Every state the walk visits therefore has A > 0, every CLOSE factor on its path is positive, and the drawn chain has
// weight > 0 -- pure erasure is exact, and so is a subnormal s, where u * s rounds back up to s and the first compare alone would decline a forced
// branch.  In the normal range the second compare of either rule is implied by the first (u <= 1 - 2^-53): no draw there depends on it.  THE LAW is a
// question of range: below kSampleFloor the pairs are rounded subnormals and their ratios are no longer the law, so check_sample_z refuses by name.
// The kernels (class_sample.hip) and the twin below run the same single multiplies, adds and compares -- both built without floating-point
// contraction -- and agree byte for byte.
//
// THE JOB is what one record serves.  With nothing held it is the (syndrome, class) pair: all K samples of the pair walk one record.  With held
// generators it is the (syndrome, class, sample) triple: every sample picks its own h* and gets its own forward sweep under it -- 2^-n_held of a
// class sweep.  In posterior mode only the drawn classes' jobs exist.  A record is n_forget * 2^(width - 1) * 16 bytes (15 MiB at rotated L = 11);
// sample_launch_group bounds the records of one launch by kSampleWorkspaceBytes and the samples of one launch by kLaunchSamples, whatever N and K.
//
// Refused, before a device is looked for, under the entry point's name: what build_cut_plan refuses, with its code; a weight that is negative or
// not finite, four zero weights; K = 0 or K >= 2^32; syndrome indices past 32 bits; a mode other than 0 and 1.  Refused by name once Z is known: in
// every-class mode a class whose Z_c is 0, not finite or below 2^-960 (row and class), in posterior mode a row whose total is.
#pragma once
#include "class_minplus_trace.hpp"   // forget_generators, remove_bit, unpack_chain
#include "class_sample_rule.hpp"     // what the cut route and the tiled route (class_sample_tiled.hpp) share: the uniforms, the checks, the decisions

#include <cstring>

namespace qecmc {
namespace sample {

constexpr uint64_t kSampleWorkspaceBytes = 512ull << 20;     // the records of one launch
constexpr uint32_t kLaunchSamples = 1u << 18;                // the samples of one pick / walk launch: their chains are 64 MiB on the device at most
constexpr int kMaxWords = 8;                                 // packed words of a chain a walk lane keeps in registers: rotated L = 11 has 8

struct SamplePlan {
    sweep::CutPlan cut;                 // refusal: cut.plan.refusal, prefixed with the entry point's name
    int n_forget = 0;
    std::vector<int> forget_gen;        // [n_forget]: the table index of the generator FORGET fi retires, in stream order
    std::vector<uint32_t> forget_words; // [n_forget][W]: that generator as packed state words, 2 bits per qubit
};

// build_cut_plan -- the sum-product plan, unchanged -- with its refusals under `name`, and the generator every FORGET retires
inline SamplePlan build_sample_plan(int code, int L, int lds_width, const char *name = "qecmc_class_sample")
{
    SamplePlan sp;
    sp.cut = sweep::build_cut_plan(code, L, lds_width);
    sweep::Plan &p = sp.cut.plan;
    if (p.refusal.code) { p.refusal = named(name, p.refusal); return sp; }
    const bool ok = minplus::forget_generators(sp.cut, code, L, sp.forget_gen, sp.forget_words);
    sp.n_forget = (int)sp.forget_gen.size();
    if (!ok || p.W > kMaxWords)
        p.refusal = named(name, refuse_params(QECMC_ERR_UNSUPPORTED, "internal: the stream of code %d at L=%d does not retire every generator once, or a chain takes more than %d words",
                                              code, L, kMaxWords));
    return sp;
}

// the record of one job, in pairs and in bytes
inline uint64_t sample_pairs_per_job(int n_forget, int width) { return (uint64_t)n_forget << (width - 1); }
inline uint64_t sample_bytes_per_job(const SamplePlan &sp) { return sample_pairs_per_job(sp.n_forget, sp.cut.plan.width) * sizeof(PairRecord); }

// How a call becomes launches.  syndromes: cut_launch_group, and with nothing held few enough that every pair of the group has its record at once
// (never 0: the largest accepted record times 16 classes stays below the workspace); k_chunk: samples per (syndrome, class) of one pick / walk
// launch, so that syndromes * ncls * k_chunk stays within kLaunchSamples (never 0); jobs: the records of one record launch.
struct LaunchGroup { uint32_t syndromes, k_chunk, jobs; };
inline LaunchGroup sample_launch_group(uint64_t N, int ncls, int n_held, uint64_t K, uint64_t bytes_per_job)
{
    LaunchGroup g;
    g.syndromes = sweep::cut_launch_group(N, ncls, n_held);
    uint64_t cap = kSampleWorkspaceBytes / (bytes_per_job ? bytes_per_job : 1ull);
    if (cap < 1ull) cap = 1ull;
    if (n_held == 0 && cap / (uint64_t)ncls < g.syndromes) g.syndromes = cap / (uint64_t)ncls < 1ull ? 1u : (uint32_t)(cap / (uint64_t)ncls);
    uint64_t kc = kLaunchSamples / ((uint64_t)g.syndromes * (uint64_t)ncls);
    if (kc < 1ull) kc = 1ull;
    g.k_chunk = (uint32_t)(K && K < kc ? K : kc);
    g.jobs = n_held == 0 ? g.syndromes * (uint32_t)ncls : (uint32_t)(cap < sweep::kCutGridMax ? cap : sweep::kCutGridMax);
    return g;
}

// ---------------------------------------------------------------- the twin
// step 3: the Decide of host_ops that keeps (on, s)
struct Recorder {
    PairRecord *R;
    uint32_t half;                      // 2^(width - 1)
    int fi = 0;
    void begin(uint32_t) {}
    void at(uint32_t h, double off, double on) { R[(size_t)fi * half + h] = PairRecord{on, off + on}; }
    void end() { ++fi; }
};

// the factors of a CLOSE: tab[q * stride + idx] -- stride 0: the four of the call, 4: the row of a site table -- in (x, z) order
struct Factors { const double *tab; size_t stride; };

// the forward sweep of one job with its record.  A: 2^width doubles, R: sample_pairs_per_job pairs, both dirty allowed -> the unscaled partial
inline double record_one(const SamplePlan &sp, const uint32_t *rep, const Factors &fc, double *A, PairRecord *R)
{
    const sweep::Plan &p = sp.cut.plan;
    A[0] = 1.0;
    sweep::host_ops(p.ops.data(), p.n_ops, rep, A, [&](double a, uint32_t q, uint32_t idx) { return a * fc.tab[(size_t)q * fc.stride + idx]; },
                    [](double a, double b) { return a + b; }, Recorder{R, 1u << (p.width - 1)});
    return A[0];
}

// step 4.  chain: W packed words, cut_representative(cp, rep, h*) on entry, the sample on return -> the f the walk ends at (0)
inline uint32_t sample_walk(const SamplePlan &sp, const PairRecord *R, uint64_t k, uint32_t syndrome, uint32_t stream, uint64_t seed, uint32_t *chain)
{
    using namespace sweep;
    const Plan &p = sp.cut.plan;
    const size_t half = (size_t)1 << (p.width - 1);
    uint32_t f = 0;
    int fi = sp.n_forget;
    for (int o = p.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = p.ops[(size_t)o * kOpWords], kind = w0 & 15u, slot = (w0 >> 4) & 15u, bit = 1u << slot;
        if (kind == kIntro) f &= ~bit;
        else if (kind == kForget) {
            --fi;
            const PairRecord r = R[(size_t)fi * half + minplus::remove_bit(f, slot)];
            const double u = draw_u53(k, 1u + ((uint32_t)fi >> 1), (uint32_t)fi & 1u, syndrome, stream, seed);
            if (take_branch(u, r.on, r.s)) {
                f |= bit;
                for (int w = 0; w < p.W; ++w) chain[w] ^= sp.forget_words[(size_t)fi * p.W + w];
            }
        }
    }
    return f;
}

// The twin.  chains uint8[N][nq]; w4[4] (I, X, Y, Z), or wq double[wq_rows][nq][4] where w4 is NULL -> mode 0: chain_out uint8[N][ncls][K][nq];
// mode 1: chain_out uint8[N][K][nq] and class_out int32[N][K]; z_out double[N][ncls] in both.  The arguments are checked by the caller; the refusal
// returned is the one Z decides.  The partials of one syndrome are spread over host threads as sweep_cut_host spreads them.
inline Refusal sample_host(const SamplePlan &sp, const char *name, uint64_t N, const uint8_t *chains, const double *w4, const double *wq, uint64_t wq_rows, uint64_t K,
                           uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out, unsigned threads = 0)
{
    const sweep::CutPlan &cp = sp.cut;
    const sweep::Plan &p = cp.plan;
    sweep::Plan unscaled = p;
    unscaled.scale = 1.0;                                                       // (A[0] * 1.0 is A[0])
    const uint32_t n_h = 1u << cp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = sweep::host_threads(threads, n_work, n_work, cp.n_held == 0);
    const size_t row = (size_t)p.nq * 4u;
    std::vector<double> wxz(w4 ? 4u : row), P((size_t)n_work), fold((size_t)n_h), A((size_t)1 << p.width);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W), chain((size_t)p.W);
    std::vector<PairRecord> R((size_t)sample_pairs_per_job(sp.n_forget, p.width));
    std::vector<int32_t> cls((size_t)(mode ? K : 0));
    if (w4) sweep::weights_xz(w4, wxz.data());
    const Factors fc{wxz.data(), w4 ? 0u : 4u};
    for (uint64_t s = 0; s < N; ++s) {
        const uint32_t syndrome = first_syndrome + (uint32_t)s;
        if (!w4 && (s == 0 || wq_rows != 1)) sweep::site_rows_xz(wq + (wq_rows == 1 ? 0u : s) * row, 1, p.nq, wxz.data());
        sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        sweep::host_partials(n_work, threads, p.width, p.W, P.data(), [&](uint32_t i, uint32_t *mine, double *Amine) {
            sweep::cut_representative(cp, &reps[(size_t)(i >> cp.n_held) * p.W], i & (n_h - 1u), mine);
            return w4 ? sweep::sweep_one(unscaled, mine, wxz.data(), Amine) : sweep::sweep_one_site(unscaled, mine, wxz.data(), Amine);
        });
        double *Z = z_out + s * (uint64_t)p.ncls;
        for (int c = 0; c < p.ncls; ++c) {
            std::memcpy(fold.data(), &P[(size_t)c << cp.n_held], (size_t)n_h * sizeof(double));
            Z[c] = sweep::cut_reduce(fold.data(), cp.n_held, p.scale);
        }
        if (const Refusal r = check_sample_z(name, s, Z, p.ncls, mode); r.code) return r;
        if (mode)
            for (uint64_t k = 0; k < K; ++k) class_out[s * K + k] = cls[(size_t)k] = (int32_t)pick_running(Z, (uint32_t)p.ncls, draw_u53(k, 0u, 0u, syndrome, (uint32_t)p.ncls, seed));
        for (int c = 0; c < p.ncls; ++c) {
            bool recorded = false;                                              // (nothing held: one record serves every sample of the pair)
            for (uint64_t k = 0; k < K; ++k) {
                if (mode && cls[(size_t)k] != c) continue;
                if (cp.n_held > 0) {
                    const uint32_t pick = pick_running(&P[(size_t)c << cp.n_held], n_h, draw_u53(k, 0u, 0u, syndrome, (uint32_t)c, seed));
                    sweep::cut_representative(cp, &reps[(size_t)c * p.W], pick, rep.data());
                    record_one(sp, rep.data(), fc, A.data(), R.data());
                } else if (!recorded) {
                    std::memcpy(rep.data(), &reps[(size_t)c * p.W], (size_t)p.W * sizeof(uint32_t));
                    record_one(sp, rep.data(), fc, A.data(), R.data());
                    recorded = true;
                }
                chain = rep;
                sample_walk(sp, R.data(), k, syndrome, (uint32_t)c, seed, chain.data());
                const uint64_t at = mode ? s * K + k : (s * (uint64_t)p.ncls + (uint64_t)c) * K + k;
                minplus::unpack_chain(chain.data(), p.nq, chain_out + at * (uint64_t)p.nq);
            }
        }
    }
    return {};
}

}  // namespace sample

// class_sample.hip: all pointers are device pointers.  ops, held and reps as class_sweep_cut.hip takes them; forget_words uint32[n_forget][W].
// The samples of one launch are numbered [s][c][kk] (mode 0) or [s][kk] (mode 1), kk < k_chunk, sample k = k0 + kk; pair = s * ncls + c.
struct SampleArgs {
    int ncls, W, width, n_ops, n_held, n_forget, nq, per_syndrome, mode;
    uint32_t seed_lo, seed_hi, syndrome0;   // syndrome0: the global index of the launch group's first syndrome
    uint32_t k0, k_chunk, n_samples;
    double wxz[4];
};
hipError_t class_sample_allow_lds(int width, int site);    // hipSuccess: the record kernel (uniform / site) can be launched with a state vector of this width
// k_class_sample_pick, after the partials P double[S * ncls][2^n_held] (left unfolded) and z double[S * ncls]: per sample its pair, its h* and, in
// mode 1, its class -- cls int32[n_samples] (mode 1 only), spair and sh uint32[n_samples].  The launch checks what the kernel reads (ncls, n_held, mode,
// k_chunk, n_samples) and nothing of the plan: the tiled route launches it too
hipError_t launch_sample_pick(const SampleArgs &a, const double *P, const double *z, int32_t *cls, uint32_t *spair, uint32_t *sh, hipStream_t stream);
// k_class_sample_record / _site: job j < jobs sweeps pair job_pair[j] under job_h[j] (NULL: 0) and writes record j of R -- PairRecord[jobs][n_forget][2^(width-1)],
// scratch, dirty allowed.  wq: NULL for the four weights of a.wxz, else double[per_syndrome ? S : 1][nq][4] in (x, z) order, 32-byte aligned
hipError_t launch_sample_record(const SampleArgs &a, uint32_t jobs, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const double *wq, const uint32_t *job_pair,
                                const uint32_t *job_h, sample::PairRecord *R, hipStream_t stream);
// k_class_sample_walk, after the record kernel on the same stream: samples [first, first + count) of the launch, one lane each; the record of sample i
// is rec_of_pair[spair[i]], or i - first where rec_of_pair is NULL (a job per sample).  chain_out uint8[n_samples][nq]
hipError_t launch_sample_walk(const SampleArgs &a, uint32_t first, uint32_t count, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *forget_words,
                              const uint32_t *spair, const uint32_t *sh, const uint32_t *rec_of_pair, const sample::PairRecord *R, uint32_t records, uint8_t *chain_out,
                              hipStream_t stream);

}  // namespace qecmc
