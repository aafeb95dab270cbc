// Exact chains of every class on the state vector tiled over HBM: forward filtering and backward sampling (class_sample.hpp's RULE) on the plans of
// class_sweep_tiled.hpp -- xzzx / rotated L = 13 .. 17 at the default cap, L = 21, planar L = 8 .. 12 and the toric code at L = 7 under a raised one.
// The contract is qecmc_class_sample's, stated in the coordinates of the WIDE stream, so that nothing in a sample depends on the tiling.
//
// THE RULE, for syndrome s (global index first_syndrome + s), class c, sample k, with the tiled plan tp of (code, L, hbm_width, tile_width), the class
// representative rep_c and the factors w (four per call, or a site table).  The uniforms are class_sample_rule.hpp's:
// u53(block, j) of philox_block(k << 16 | block, 0x53, first_syndrome + s, stream, seed).
//     1. PARTIALS   P[h] under every assignment h of the held generators, by qecmc_class_sweep_tiled's kernels, unchanged; Z_c = cut_reduce of them:
//                   qecmc_class_sweep_tiled's bits.
//     2. PICK       (n_held > 0 only; else h* = 0 and no draw is spent)  pick_running of P[0 ..] under u = u53(0, 0) on stream c: both compares.
//     3. RECORD     the wide op stream once more under h*, one unit per job; at FORGET number fi (its ordinal in the wide stream), for every live f with
//                   the slot bit clear, the pair (on, s) = (A[f | bit], A[f] + A[f | bit]) -- s is the very double the FORGET leaves in A[f].
//     4. WALK       f = 0, chain = tiled_representative(tp, rep_c, h*); through the wide ops in reverse: FORGET: (on, s) at (fi, f),
//                   u = u53(1 + (fi >> 1), fi & 1) on stream c, the generator is taken iff u * s < on || on == s: f |= bit, chain ^= forget_words[fi];
//                   INTRO: f &= ~bit; CLOSE: nothing.  The walk ends at f == 0.
//     5. RESULT     the chain as bytes uint8[nq]; a cell no generator touches keeps the representative's byte.
// POSTERIOR MODE draws the class first on stream ncls, as class_sample.hpp does.  A sample is a function of (seed, first_syndrome + s, c, k, wide stream
// and holds, representative, weights) alone: not of tile_width, N, K or the pass grouping; and wherever the tiled plan's stream and holds are the cut
// plan's (nothing held and width <= 13; hbm_width = the cut plan's lds_width) the chains are qecmc_class_sample's byte for byte.  Support and range
// are class_sample.hpp's: a drawn chain has weight > 0 at every range; check_sample_z refuses below 2^-960 by row and class.
//
// THE JOB is what one record serves: with nothing held the (syndrome, class) pair -- all K samples walk one record --, with held generators the
// (syndrome, class, sample) triple; in posterior mode only the drawn classes' jobs exist.
//
// THE RECORD ON THE DEVICE.  FORGET fi lies in one segment, with tile bits T and fixed_live = live & ~T.  The workgroup of live tile x stores, for
// local half-index h (local f = insert_zero(h, local slot)), one 16-byte pair at R[job in pass][pair_off[fi] + x * 2^(tile_width - 1) + h];
// pair_off[fi + 1] = pair_off[fi] + n_tiles(segment of fi) * 2^(tile_width - 1), bytes_per_job = 16 * pair_off[n_forget]: only live tiles take space.
// The walk finds its pair from the global f: x = bits_extract(f, fixed_live), l = bits_extract(f, T), h = remove_bit(l, local slot), through
// forget_tile[fi] = {T, fixed_live, local slot, pair_off[fi]}, built on the host.  It reads only pairs the record kernels wrote in the same call -- f
// is a submask of the live slots at every step --, so the block and LDS may be dirty.  The block is its own, per device, grown on demand under the
// tiled workspace's lock up to the call's cap (record_bytes; 0: kTiledSampleRecordBytes); a plan whose single job passes the cap is refused by name
// with the bytes it needs.  bytes_per_job is 128 times class_minplus_tiled_trace.hpp's bytes_per_pair wherever tile_width >= 7 (a pair for a bit).
//
// THE TWIN (sample_tiled_host) is plain C++ written apart from the device loop: a flat state vector, the wide stream, the pairs in a flat array indexed
// by (fi, remove_bit(f, slot)) in GLOBAL coordinates and a Philox of its own (draw_u53) -- it knows nothing of tiles, segments or forget_tile.
#pragma once
#include "class_minplus_trace.hpp"   // remove_bit, unpack_chain
#include "class_sample_rule.hpp"
#include "class_sweep_tiled.hpp"

namespace qecmc {
namespace sample {

constexpr uint64_t kTiledSampleRecordBytes = 4ull << 30;      // the records of one record pass, where the call names no cap
constexpr uint64_t kTiledSampleRecordBytesMax = 64ull << 30;  // the largest cap a call may name: 2^32 pairs, what a 32-bit pair_off addresses
constexpr int kTiledForgetWords = 4;                          // {T, fixed_live, local slot, pair_off}
constexpr int kTiledMaxWords = 28;                            // packed words of a chain a walk lane keeps in its LDS column: rotated L = 21 has 28
constexpr uint32_t kTiledLaunchSamples = 1u << 18;            // the samples of one pick / walk launch (class_sample.hpp's kLaunchSamples)

struct TiledSamplePlan {
    sweep::TiledPlan tiled;             // refusal: tiled.plan.refusal, under the entry point's name
    int n_forget = 0;
    uint64_t pairs_per_job = 0;         // pair_off[n_forget]
    std::vector<int> forget_gen;        // [n_forget]: the table index of the generator FORGET fi retires, in stream order
    std::vector<uint32_t> forget_words; // [n_forget][W]: that generator as packed state words (held_words' layout)
    std::vector<uint32_t> forget_tile;  // [n_forget][kTiledForgetWords]
    std::vector<uint64_t> pair_off;     // [n_forget + 1]
    std::vector<uint32_t> seg_forget;   // [n_segments]: the ordinal of the segment's first FORGET (n_forget where none follows)
};

inline uint64_t tiled_sample_bytes_per_job(const TiledSamplePlan &tsp) { return tsp.pairs_per_job * sizeof(PairRecord); }

// the cap of a call: 0 is the default; a value past kTiledSampleRecordBytesMax is refused by name
inline Refusal check_record_bytes(const char *name, uint64_t record_bytes, uint64_t *cap)
{
    *cap = record_bytes ? record_bytes : kTiledSampleRecordBytes;
    if (record_bytes > kTiledSampleRecordBytesMax)
        return named(name, refuse_params(QECMC_ERR_INVALID, "record_bytes=%llu: the cap of the record block is 1 .. %llu bytes, or 0 for the default of %llu",
                                         (unsigned long long)record_bytes, (unsigned long long)kTiledSampleRecordBytesMax, (unsigned long long)kTiledSampleRecordBytes));
    return {};
}

// the jobs of one record pass: what the state workspace takes, what the record block takes under `cap` bytes, and what is left; never 0
inline uint32_t tiled_sample_pass_jobs(int state_bits, uint64_t bytes_per_job, uint64_t jobs_left, uint64_t cap = kTiledSampleRecordBytes)
{
    uint64_t n = sweep::tiled_pass_units(state_bits);
    const uint64_t fit = cap / (bytes_per_job ? bytes_per_job : 1ull);
    if (fit < n) n = fit;
    if (jobs_left < n) n = jobs_left;
    return n < 1ull ? 1u : (uint32_t)n;
}

// build_tiled_plan under the entry point's name, the generator every FORGET of its final wide stream retires, and where the device keeps the pairs of
// each.  Refused: what build_tiled_plan refuses, with its code, and a plan whose single job takes more than `cap` bytes of record, by name.  The
// tables of a plan refused for the cap alone are complete (n_forget, pair_off): the info call reports what the plan would take.
inline TiledSamplePlan build_tiled_sample_plan(int code, int L, int hbm_width, int tile_width, const char *entry = "qecmc_class_sample_tiled",
                                               uint64_t cap = kTiledSampleRecordBytes)
{
    TiledSamplePlan tsp;
    tsp.tiled = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    sweep::TiledPlan &tp = tsp.tiled;
    sweep::Plan &p = tp.plan;
    if (p.refusal.code) { p.refusal = named(entry, p.refusal); return tsp; }
    // ---- the generators, from the final stream: the one build_tiled_plan encoded (build_stream is a function of (code, L, holds))
    std::vector<char> held((size_t)p.n_gen, 0);
    for (const int g : tp.held) held[(size_t)g] = 1;
    sweep::Trace tr;
    const sweep::Stream st = sweep::build_stream(code, L, held, &tr);
    const correct::Table &ct = st.table;
    std::vector<int> at_op((size_t)p.n_ops, -1);
    bool ok = st.head.refusal.code == 0 && (int)st.ops.size() == p.n_ops && (int)tp.ops.size() == p.n_ops * sweep::kTiledOpWords;
    for (int g = 0; ok && g < p.n_gen; ++g) {
        const int at = tr.forget_at[(size_t)g];
        if (held[(size_t)g]) { ok = at < 0; continue; }
        ok = at >= 0 && at < p.n_ops && at_op[(size_t)at] < 0 && (tp.ops[(size_t)at * sweep::kTiledOpWords] & 15u) == sweep::kForget;
        if (ok) at_op[(size_t)at] = g;
    }
    const uint64_t half = 1ull << (tp.tile_width - 1);
    uint64_t off = 0;
    for (size_t s = 0; ok && s < tp.segments.size(); ++s) {
        const sweep::Segment &sg = tp.segments[s];
        tsp.seg_forget.push_back((uint32_t)tsp.forget_gen.size());
        for (uint32_t o = sg.op_first; ok && o < sg.op_first + sg.op_count; ++o) {
            const uint32_t w0 = tp.ops[(size_t)o * sweep::kTiledOpWords];
            if ((w0 & 15u) != sweep::kForget) continue;
            const int g = at_op[(size_t)o];
            const uint32_t slot = (w0 >> 4) & 31u;
            if (g < 0 || !((sg.tile >> slot) & 1u)) { ok = false; break; }
            tsp.forget_gen.push_back(g);
            std::vector<uint32_t> words((size_t)ct.W, 0u);
            for (int i = 0; i < 4; ++i) {
                const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
                words[site >> 4] ^= pauli << ((site & 15u) * 2u);               // (Pauli values XOR as the Pauli product)
            }
            tsp.forget_words.insert(tsp.forget_words.end(), words.begin(), words.end());
            // (pair_off as 32 bits: what the walk reads is used only under a cap of 2^32 pairs at most, where every offset of a FORGET is below 2^32)
            const uint32_t row[kTiledForgetWords] = {sg.tile, sg.live & ~sg.tile, sweep::popcount32(sg.tile & ((1u << slot) - 1u)), (uint32_t)off};
            tsp.forget_tile.insert(tsp.forget_tile.end(), row, row + kTiledForgetWords);
            tsp.pair_off.push_back(off);
            off += (uint64_t)sg.n_tiles * half;
        }
    }
    tsp.pair_off.push_back(off);
    tsp.n_forget = (int)tsp.forget_gen.size();
    tsp.pairs_per_job = off;
    if (!ok || tsp.n_forget != p.n_gen - tp.n_held || tsp.n_forget < 1 || p.W > kTiledMaxWords)
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "%s: internal: the stream of code %d at L=%d does not retire every generator once, or a chain takes more than %d words",
                                  entry, code, L, kTiledMaxWords);
    else if (cap > kTiledSampleRecordBytesMax || off * sizeof(PairRecord) > cap)
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "%s: the record of one job of code %d at L=%d takes %llu bytes at tile_width %d, more than the %llu of the record block "
                                                         "(record_bytes)", entry, code, L, (unsigned long long)(off * sizeof(PairRecord)), tp.tile_width, (unsigned long long)cap);
    return tsp;
}

// check_sample_site for a tiled plan, whose stream is the wide one (plan.ops stays empty)
inline Refusal check_sample_tiled_site(const char *name, uint64_t N, const double *wq, uint64_t wq_rows, const sweep::TiledPlan &tp)
{
    if (const Refusal r = sweep::check_site_rows(N, wq_rows); r.code) return named(name, r);
    return N ? named(name, sweep::check_site_weights(wq, wq_rows, tp.plan.nq, sweep::closed_qubits(tp.ops, tp.plan.nq))) : Refusal{};
}

// ---------------------------------------------------------------- the twin
// step 3 on the host: the wide stream over the flat A[2^width] (dirty allowed) under the factors tab[q * stride + idx] (stride 0: the four of the call,
// 4: a row of a site table, both in (x, z) order), and the pair of every FORGET fi and live f at R[fi * 2^(width - 1) + remove_bit(f, slot)] in global
// coordinates (dirty allowed: dead f keep nothing and are never read) -> the unscaled partial
inline double record_one_wide(const sweep::TiledPlan &tp, const uint32_t *rep, const double *tab, size_t stride, double *A, PairRecord *R)
{
    const size_t half = (size_t)1 << (tp.plan.width - 1);
    size_t fi = 0;
    A[0] = 1.0;
    for (int o = 0; o < tp.plan.n_ops; ++o) {
        const uint32_t *op = &tp.ops[(size_t)o * sweep::kTiledOpWords];
        const uint32_t kind = op[0] & 15u, slot = (op[0] >> 4) & 31u, bit = 1u << slot, mask = op[1];
        uint32_t f = 0;
        if (kind == sweep::kClose) {
            const uint32_t q = op[3], cq = sweep::pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
            do {
                uint32_t idx = cq;
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (op[2] >> (8 * j)) & 0xFFu;
                    if ((f >> (pr & 31u)) & 1u) idx ^= pr >> 5;
                }
                A[f] = A[f] * tab[(size_t)q * stride + idx];
                f = (f - mask) & mask;
            } while (f);
        } else if (kind == sweep::kIntro) {
            do { A[f | bit] = A[f]; f = (f - mask) & mask; } while (f);
        } else {
            PairRecord *mine = R + fi++ * half;
            do {
                const double off = A[f], on = A[f | bit], s = off + on;
                mine[minplus::remove_bit(f, slot)] = PairRecord{on, s};
                A[f] = s;
                f = (f - mask) & mask;
            } while (f);
        }
    }
    return A[0];
}

// step 4 on the host, in global coordinates.  chain: W packed words, tiled_representative(tp, rep, h*) on entry, the sample on return -> the f the
// walk ends at (0)
inline uint32_t sample_tiled_walk(const TiledSamplePlan &tsp, const PairRecord *R, uint64_t k, uint32_t syndrome, uint32_t stream, uint64_t seed, uint32_t *chain)
{
    const sweep::TiledPlan &tp = tsp.tiled;
    const size_t half = (size_t)1 << (tp.plan.width - 1);
    uint32_t f = 0;
    int fi = tsp.n_forget;
    for (int o = tp.plan.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = tp.ops[(size_t)o * sweep::kTiledOpWords], kind = w0 & 15u, slot = (w0 >> 4) & 31u, bit = 1u << slot;
        if (kind == sweep::kIntro) f &= ~bit;
        else if (kind == sweep::kForget) {
            --fi;
            const PairRecord r = R[(size_t)fi * half + minplus::remove_bit(f, slot)];
            const double u = draw_u53(k, 1u + ((uint32_t)fi >> 1), (uint32_t)fi & 1u, syndrome, stream, seed);
            if (take_branch(u, r.on, r.s)) {
                f |= bit;
                for (int w = 0; w < tp.plan.W; ++w) chain[w] ^= tsp.forget_words[(size_t)fi * tp.plan.W + w];
            }
        }
    }
    return f;
}

// The twin of qecmc_class_sample_tiled (w4 given) and qecmc_class_sample_tiled_site (w4 NULL, wq double[wq_rows][nq][4]).  chains uint8[N][nq] ->
// mode 0: chain_out uint8[N][ncls][K][nq]; mode 1: chain_out uint8[N][K][nq] and class_out int32[N][K]; z_out double[N][ncls] in both.  The arguments
// are checked by the caller; the refusal returned is the one Z decides.  The partials of one syndrome are spread over host threads as
// sweep_tiled_host spreads them; the record of a job is one more pass on the calling thread.
inline Refusal sample_tiled_host(const TiledSamplePlan &tsp, const char *name, uint64_t N, const uint8_t *chains, const double *w4, const double *wq, uint64_t wq_rows,
                                 uint64_t K, uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out, unsigned threads = 0)
{
    const sweep::TiledPlan &tp = tsp.tiled;
    const sweep::Plan &p = tp.plan;
    const uint32_t n_h = 1u << tp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = sweep::host_threads(threads, n_work, sweep::tiled_pass_units(p.width), p.width < 12);
    const size_t row = (size_t)p.nq * 4u, stride = w4 ? 0u : 4u;
    std::vector<double> wxz(w4 ? 4u : row), P((size_t)n_work), fold((size_t)n_h), A((size_t)1 << p.width);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W), chain((size_t)p.W);
    std::vector<PairRecord> R((size_t)tsp.n_forget << (p.width - 1));
    std::vector<int32_t> cls((size_t)(mode ? K : 0));
    if (w4) sweep::weights_xz(w4, wxz.data());
    for (uint64_t s = 0; s < N; ++s) {
        const uint32_t syndrome = first_syndrome + (uint32_t)s;
        if (!w4 && (s == 0 || wq_rows != 1)) sweep::site_rows_xz(wq + (wq_rows == 1 ? 0u : s) * row, 1, p.nq, wxz.data());
        sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        sweep::host_partials(n_work, threads, p.width, p.W, P.data(), [&](uint32_t i, uint32_t *mine, double *Amine) {
            sweep::tiled_representative(tp, &reps[(size_t)(i >> tp.n_held) * p.W], i & (n_h - 1u), mine);
            return w4 ? sweep::sweep_one_wide(tp, mine, wxz.data(), Amine) : sweep::sweep_one_wide_site(tp, mine, wxz.data(), Amine);
        });
        double *Z = z_out + s * (uint64_t)p.ncls;
        for (int c = 0; c < p.ncls; ++c) {
            std::memcpy(fold.data(), &P[(size_t)c << tp.n_held], (size_t)n_h * sizeof(double));
            Z[c] = sweep::cut_reduce(fold.data(), tp.n_held, p.scale);
        }
        if (const Refusal r = check_sample_z(name, s, Z, p.ncls, mode); r.code) return r;
        if (mode)
            for (uint64_t k = 0; k < K; ++k) class_out[s * K + k] = cls[(size_t)k] = (int32_t)pick_running(Z, (uint32_t)p.ncls, draw_u53(k, 0u, 0u, syndrome, (uint32_t)p.ncls, seed));
        for (int c = 0; c < p.ncls; ++c) {
            bool recorded = false;                                              // (nothing held: one record serves every sample of the pair)
            for (uint64_t k = 0; k < K; ++k) {
                if (mode && cls[(size_t)k] != c) continue;
                if (tp.n_held > 0) {
                    const uint32_t pick = pick_running(&P[(size_t)c << tp.n_held], n_h, draw_u53(k, 0u, 0u, syndrome, (uint32_t)c, seed));
                    sweep::tiled_representative(tp, &reps[(size_t)c * p.W], pick, rep.data());
                    record_one_wide(tp, rep.data(), wxz.data(), stride, A.data(), R.data());
                } else if (!recorded) {
                    std::memcpy(rep.data(), &reps[(size_t)c * p.W], (size_t)p.W * sizeof(uint32_t));
                    record_one_wide(tp, rep.data(), wxz.data(), stride, A.data(), R.data());
                    recorded = true;
                }
                chain = rep;
                sample_tiled_walk(tsp, R.data(), k, syndrome, (uint32_t)c, seed, chain.data());
                const uint64_t at = mode ? s * K + k : (s * (uint64_t)p.ncls + (uint64_t)c) * K + k;
                minplus::unpack_chain(chain.data(), p.nq, chain_out + at * (uint64_t)p.nq);
            }
        }
    }
    return {};
}

}  // namespace sample

// class_sample_tiled.hip: all pointers are device pointers.  dev_ops, held, reps as class_sweep_tiled.hip takes them; wide_ops
// uint32[n_ops][kTiledOpWords]; forget_tile uint32[n_forget][kTiledForgetWords]; forget_words uint32[n_forget][W]; work double[jobs][2^state_bits] and
// R PairRecord[jobs][pairs_per_job]: the state vectors and the records of one record pass, both dirty; wq as the site sweep's.
struct SampleTiledArgs {
    uint32_t unit_first, units;        // the jobs of this pass: rows unit_first .. unit_first + units of the job table
    int W, n_held, state_bits, tile_width;
    uint32_t op_first, op_count, tile, fixed_live, local_in, local_out, n_tiles, first, last;
    uint32_t forget_first, n_forget;   // the ordinal of the segment's first FORGET
    uint64_t pairs_per_job;
    int ncls, nq, per_syndrome;        // the site kernel's (wxz is the uniform kernel's)
    double wxz[4];
};
// The samples of one launch are numbered [s][c][kk] (mode 0) or [s][kk] (mode 1), kk < k_chunk, sample k = k0 + kk; pair = s * ncls + c: the numbering
// of k_class_sample_pick (class_sample.hpp), whose spair and sh the walk reads.
struct SampleTiledWalkArgs {
    int ncls, W, n_held, n_ops, n_forget, nq, tile_width;
    uint32_t seed_lo, seed_hi, syndrome0, k0, k_chunk;
    uint32_t first, count;             // the samples this launch walks, one lane each
    uint32_t rec_first, records;       // the jobs whose records the block holds: a sample of another job leaves at once
    uint64_t pairs_per_job;
};
// k_class_sample_tiled_record / _record_site, segment by segment: job j of the pass sweeps pair job_pair[job_first + j] under job_h[job_first + j]
// (NULL: 0) and writes record j of R.  wxz == nullptr: the site table wq; stream order is the only synchronisation
hipError_t launch_sample_tiled_record(const sample::TiledSamplePlan &tsp, const double *wxz, int per_syndrome, uint32_t job_first, uint32_t jobs, const uint32_t *dev_ops,
                                      const uint32_t *held, const uint32_t *reps, const double *wq, const uint32_t *job_pair, const uint32_t *job_h, const uint32_t *forget_tile,
                                      double *work, sample::PairRecord *R, hipStream_t stream);
// k_class_sample_tiled_walk, after the record kernels of the pass on the same stream: the job of sample i is rec_of_pair[spair[i]], or i where
// rec_of_pair is NULL (a job per sample).  chain_out uint8[n_samples][nq]
hipError_t launch_sample_tiled_walk(const sample::TiledSamplePlan &tsp, const SampleTiledWalkArgs &t, const uint32_t *wide_ops, const uint32_t *held, const uint32_t *reps,
                                    const uint32_t *forget_words, const uint32_t *forget_tile, const uint32_t *spair, const uint32_t *sh, const uint32_t *rec_of_pair,
                                    const sample::PairRecord *R, uint8_t *chain_out, hipStream_t stream);

}  // namespace qecmc
