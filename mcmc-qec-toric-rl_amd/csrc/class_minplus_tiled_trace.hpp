// A shortest chain of every class on the state vector tiled over HBM: the traceback of class_minplus_trace.hpp on the plans of class_sweep_tiled.hpp --
// xzzx / rotated L = 13 .. 21, planar L = 8 .. 12, the toric code at L = 7.  The contract is class_minplus_trace.hpp's, stated in the coordinates of the
// WIDE stream, so that nothing in it depends on the tiling.  For one (syndrome, class) pair, with tiled plan tp and class representative rep:
//     1. PARTIALS   P[h] under every assignment h of the held generators: what qecmc_class_minplus_tiled computes, by its kernels, unchanged.
//     2. PICK       h* = the lowest h whose P[h] has the least cost (pick_assignment; k_minplus_pick on the device).  Only costs are compared.
//     3. FORWARD    the wide op stream once more under h*, one unit per PAIR; at every FORGET and every live f with the slot bit clear,
//                       take = cost(A[f | bit]) < cost(A[f])            -- strict: a tie leaves the generator off.
//     4. WALK       f = 0, chain = tiled_representative(tp, rep, h*); through the wide ops in reverse: FORGET number fi: where the decision of (fi, f)
//                   is set, f |= bit and chain ^= forget_words[fi]; INTRO: f &= ~bit; CLOSE: nothing.  The walk ends at f == 0.
//     5. RESULT     the chain as bytes uint8[nq]; a cell no generator touches keeps the representative's byte.
// The chain is therefore a pure function of (wide stream, holds, representative, costs): it does not depend on tile_width, and wherever the tiled
// plan's stream and holds are the cut plan's (nothing held and width <= 13; hbm_width = the cut plan's lds_width) it is qecmc_class_minplus_chains'
// chain byte for byte.
//
// THE DECISIONS ON THE DEVICE.  FORGET fi lies in one segment, with tile bits T and fixed_live = live & ~T.  The workgroup of live tile x ballots
// its local half-indices h (local f = insert_zero(h, local slot)) in whole waves and writes words_per_tile = max(1, 2^(tile_width - 1) / 64) 64-bit
// words at D[pair in pass][off[fi] + x * words_per_tile + (h >> 6)], bit h & 63.  Only live tiles are launched, so only live tiles take space:
// off[fi + 1] = off[fi] + n_tiles(segment of fi) * words_per_tile, and bytes_per_pair = 8 * off[n_forget].  The walk finds its bit from the global f:
// x = bits_extract(f, fixed_live), l = bits_extract(f, T), h = remove_bit(l, local slot).  forget_tile[fi] = {T, fixed_live, local slot, off[fi]} is
// built on the host; every segment's launch carries the ordinal of its first FORGET.  The walk reads only bits the trace kernels wrote in the same
// call -- f is a submask of the live slots at every step, whatever the bits say -- so the decision block and LDS may be dirty, like the state
// workspace.  bytes_per_pair at the defaults: rotated L = 13: 496 896, L = 17: 13 082 880, L = 21: 303 650 944; planar L = 12: 258 412 928;
// toric L = 7: 77 956 992.  The block is kTiledTraceWorkspaceBytes at most; a plan whose single pair passes it is refused by name (none of the
// accepted shapes is, at any tile_width: rotated L = 21 at tile_width 4 takes 1 953 147 944).
//
// THE TWIN (minplus_tiled_trace_host, ..._site_host) is plain C++ written apart from the device loop: a flat state vector, the wide stream, and the
// decisions in a flat array indexed by (fi, remove_bit(f, slot)) in GLOBAL coordinates -- it knows nothing of tiles, segments or forget_tile.
#pragma once
#include "class_minplus_tiled.hpp"

namespace qecmc {
namespace minplus {

constexpr uint64_t kTiledTraceWorkspaceBytes = 2ull << 30;    // the decision words of one trace pass
constexpr int kForgetTileWords = 4;                           // {T, fixed_live, local slot, off}

struct TiledTracePlan {
    sweep::TiledPlan tiled;             // refusal: tiled.plan.refusal, under the entry point's name
    int n_forget = 0, words_per_tile = 1;
    uint64_t words_per_pair = 0;        // off[n_forget]
    std::vector<int> forget_gen;        // [n_forget]: the table index of the generator FORGET fi retires, in stream order
    std::vector<uint32_t> forget_words; // [n_forget][W]: that generator as packed state words (held_words' layout)
    std::vector<uint32_t> forget_tile;  // [n_forget][kForgetTileWords]
    std::vector<uint32_t> seg_forget;   // [n_segments]: the ordinal of the segment's first FORGET (n_forget where none follows)
};

constexpr int tiled_trace_words_per_tile(int tile_width) { return tile_width - 1 > 6 ? 1 << (tile_width - 1 - 6) : 1; }

inline uint64_t tiled_trace_bytes_per_pair(const TiledTracePlan &ttp) { return ttp.words_per_pair * 8ull; }

// the pairs of one trace pass: what the state workspace takes, what the decision block takes under `cap` bytes, and what is left; never 0
inline uint32_t tiled_trace_pass_pairs(int state_bits, uint64_t bytes_per_pair, uint64_t pairs_left, uint64_t cap = kTiledTraceWorkspaceBytes)
{
    uint64_t n = sweep::tiled_pass_units(state_bits);
    const uint64_t fit = cap / (bytes_per_pair ? bytes_per_pair : 1ull);
    if (fit < n) n = fit;
    if (pairs_left < n) n = pairs_left;
    return n < 1ull ? 1u : (uint32_t)n;
}

// build_tiled_plan under the entry point's name, the generator every FORGET of its final wide stream retires, and where the device keeps the
// decisions of each.  Refused: what build_tiled_plan refuses, and a plan whose single pair takes more than `cap` bytes of decisions, by name.
inline TiledTracePlan build_tiled_trace_plan(int code, int L, int hbm_width, int tile_width, const char *entry = "qecmc_class_minplus_tiled_chains",
                                             uint64_t cap = kTiledTraceWorkspaceBytes)
{
    TiledTracePlan ttp;
    ttp.tiled = build_minplus_tiled_plan(code, L, hbm_width, tile_width, entry);
    sweep::TiledPlan &tp = ttp.tiled;
    sweep::Plan &p = tp.plan;
    if (p.refusal.code) return ttp;
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
    ttp.words_per_tile = tiled_trace_words_per_tile(tp.tile_width);
    uint64_t off = 0;
    for (size_t s = 0; ok && s < tp.segments.size(); ++s) {
        const sweep::Segment &sg = tp.segments[s];
        ttp.seg_forget.push_back((uint32_t)ttp.forget_gen.size());
        for (uint32_t o = sg.op_first; ok && o < sg.op_first + sg.op_count; ++o) {
            const uint32_t w0 = tp.ops[(size_t)o * sweep::kTiledOpWords];
            if ((w0 & 15u) != sweep::kForget) continue;
            const int g = at_op[(size_t)o];
            const uint32_t slot = (w0 >> 4) & 31u;
            if (g < 0 || !((sg.tile >> slot) & 1u) || off > 0xFFFFFFFFull) { ok = false; break; }
            ttp.forget_gen.push_back(g);
            std::vector<uint32_t> words((size_t)ct.W, 0u);
            for (int i = 0; i < 4; ++i) {
                const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
                words[site >> 4] ^= pauli << ((site & 15u) * 2u);               // (Pauli values XOR as the Pauli product)
            }
            ttp.forget_words.insert(ttp.forget_words.end(), words.begin(), words.end());
            const uint32_t row[kForgetTileWords] = {sg.tile, sg.live & ~sg.tile, sweep::popcount32(sg.tile & ((1u << slot) - 1u)), (uint32_t)off};
            ttp.forget_tile.insert(ttp.forget_tile.end(), row, row + kForgetTileWords);
            off += (uint64_t)sg.n_tiles * (uint64_t)ttp.words_per_tile;
        }
    }
    ttp.n_forget = (int)ttp.forget_gen.size();
    ttp.words_per_pair = off;
    if (!ok || ttp.n_forget != p.n_gen - tp.n_held || ttp.n_forget < 1)
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "%s: internal: the stream of code %d at L=%d does not retire every generator once", entry, code, L);
    else if (off * 8ull > cap)
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "%s: the decisions of one (syndrome, class) pair of code %d at L=%d take %llu bytes at tile_width %d, more than the "
                                                         "%llu of the decision block", entry, code, L, (unsigned long long)(off * 8ull), tp.tile_width, (unsigned long long)cap);
    return ttp;
}

// the four costs of the traced entry point: check_tiled_costs and check_tiled_cost_range under its name
inline Refusal check_tiled_chain_costs(const sweep::Plan *p, const uint32_t *cost)
{
    return site_prefix(p ? check_tiled_cost_range(*p, cost) : check_tiled_costs(cost), "qecmc_class_minplus_tiled:", "qecmc_class_minplus_tiled_chains:");
}
inline Refusal check_tiled_chain_cost_rows_range(const uint8_t *cq, uint64_t rows, int nq, const std::vector<char> &named)
{
    return site_prefix(check_tiled_cost_rows_range(cq, rows, nq, named), "qecmc_class_minplus_tiled_site:", "qecmc_class_minplus_tiled_chains_site:");
}

// ---------------------------------------------------------------- the twin
constexpr int host_words_per_forget(int width) { return width - 1 > 6 ? 1 << (width - 1 - 6) : 1; }

// step 3 on the host: the wide stream over the flat A[2^width] (dirty allowed), and the decision of every FORGET fi and live f at bit h & 63 of
// D[fi * host_words_per_forget(width) + (h >> 6)], h = remove_bit(f, slot) in global coordinates (dirty allowed: a live bit is set or cleared, no other
// is touched).  close(a, q, idx): the entry after the CLOSE of qubit q at idx = x | z << 1 -> the packed partial
template <class Close> inline uint64_t minplus_one_wide_traced(const sweep::TiledPlan &tp, const uint32_t *rep, Close close, uint64_t *A, uint64_t *D)
{
    const size_t wpf = (size_t)host_words_per_forget(tp.plan.width);
    size_t fi = 0;
    A[0] = 1ull;                                                                // (0, 1)
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
                A[f] = close(A[f], q, idx);
                f = (f - mask) & mask;
            } while (f);
        } else if (kind == sweep::kIntro) {
            do { A[f | bit] = A[f]; f = (f - mask) & mask; } while (f);
        } else {
            uint64_t *mine = D + fi++ * wpf;
            do {
                const uint64_t off = A[f], on = A[f | bit];
                const uint32_t h = remove_bit(f, slot);
                const uint64_t one = 1ull << (h & 63u);
                mine[h >> 6] = (on >> kCountBits) < (off >> kCountBits) ? mine[h >> 6] | one : mine[h >> 6] & ~one;      // strict: a tie leaves the generator off
                A[f] = mp_combine(off, on);
                f = (f - mask) & mask;
            } while (f);
        }
    }
    return A[0];
}

// step 4 on the host, in global coordinates.  chain: W packed words, tiled_representative(tp, rep, h*) on entry, the traced chain on return -> the f
// the walk ends at (0)
inline uint32_t tiled_trace_walk(const TiledTracePlan &ttp, const uint64_t *D, uint32_t *chain)
{
    const sweep::TiledPlan &tp = ttp.tiled;
    const size_t wpf = (size_t)host_words_per_forget(tp.plan.width);
    uint32_t f = 0;
    int fi = ttp.n_forget;
    for (int o = tp.plan.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = tp.ops[(size_t)o * sweep::kTiledOpWords], kind = w0 & 15u, slot = (w0 >> 4) & 31u, bit = 1u << slot;
        if (kind == sweep::kIntro) f &= ~bit;
        else if (kind == sweep::kForget) {
            --fi;
            const uint32_t h = remove_bit(f, slot);
            if ((D[(size_t)fi * wpf + (h >> 6)] >> (h & 63u)) & 1ull) {
                f |= bit;
                for (int w = 0; w < tp.plan.W; ++w) chain[w] ^= ttp.forget_words[(size_t)fi * tp.plan.W + w];
            }
        }
    }
    return f;
}

// steps 2 .. 5 for the classes of one syndrome, from its partials P[ncls][2^n_held]; one_traced(rep, A, D) runs step 3
template <class OneTraced>
inline void tiled_trace_classes(const TiledTracePlan &ttp, const uint32_t *reps, const uint64_t *P, uint64_t *A, uint64_t *D, uint8_t *chain_out, OneTraced one_traced)
{
    const sweep::TiledPlan &tp = ttp.tiled;
    const sweep::Plan &p = tp.plan;
    std::vector<uint32_t> rep((size_t)p.W);
    for (int c = 0; c < p.ncls; ++c) {
        const uint32_t pick = pick_assignment(&P[(size_t)c << tp.n_held], tp.n_held);
        sweep::tiled_representative(tp, &reps[(size_t)c * p.W], pick, rep.data());
        one_traced(rep.data(), A, D);
        tiled_trace_walk(ttp, D, rep.data());
        unpack_chain(rep.data(), p.nq, chain_out + (size_t)c * (size_t)p.nq);
    }
}

// The twin of qecmc_class_minplus_tiled_chains.  chains uint8[N][nq], cost4[4] (I, X, Y, Z) -> chain_out uint8[N][ncls][nq]; cost_out uint32[N][ncls],
// count_out uint64[N][ncls] and cls int32[N] (all three nullable): minplus_tiled_host's, exactly.  The partials are threaded as there; the trace of a
// pair is one more pass on the calling thread.
inline void minplus_tiled_trace_host(const TiledTracePlan &ttp, uint64_t N, const uint8_t *chains, const uint32_t *cost4, uint8_t *chain_out, uint32_t *cost_out,
                                     uint64_t *count_out, int32_t *cls, unsigned threads = 0)
{
    const sweep::TiledPlan &tp = ttp.tiled;
    const sweep::Plan &p = tp.plan;
    uint32_t cxz[4];
    costs_xz(cost4, cxz);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W), cost((size_t)p.ncls);
    std::vector<uint64_t> P((size_t)p.ncls << tp.n_held), count((size_t)p.ncls), A((size_t)1 << p.width), D((size_t)ttp.n_forget * (size_t)host_words_per_forget(p.width));
    for (uint64_t s = 0; s < N; ++s) {
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        tiled_partials_fold(tp, reps.data(), threads, P.data(), cost.data(), count.data(), [&](const uint32_t *rep, uint64_t *Amine) { return minplus_one_wide(tp, rep, cxz, Amine); });
        tiled_trace_classes(ttp, reps.data(), P.data(), A.data(), D.data(), chain_out + s * (uint64_t)p.ncls * (uint64_t)p.nq, [&](const uint32_t *rep, uint64_t *Am, uint64_t *Dm) {
            minplus_one_wide_traced(tp, rep, [&](uint64_t e, uint32_t, uint32_t idx) { return e + ((uint64_t)cxz[idx] << kCountBits); }, Am, Dm);
        });
        for (int c = 0; c < p.ncls; ++c) {
            if (cost_out) cost_out[s * (uint64_t)p.ncls + c] = cost[(size_t)c];
            if (count_out) count_out[s * (uint64_t)p.ncls + c] = count[(size_t)c];
        }
    }
}

// The twin of qecmc_class_minplus_tiled_chains_site.  cq uint8[cq_rows][nq][4] (I, X, Y, Z), cq_rows 1 or N
inline void minplus_tiled_trace_site_host(const TiledTracePlan &ttp, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, uint8_t *chain_out,
                                          uint32_t *cost_out, uint64_t *count_out, int32_t *cls, unsigned threads = 0)
{
    const sweep::TiledPlan &tp = ttp.tiled;
    const sweep::Plan &p = tp.plan;
    const size_t row = (size_t)p.nq * 4u;
    std::vector<uint32_t> cw((size_t)p.nq), reps((size_t)p.ncls * p.W), cost((size_t)p.ncls);
    std::vector<uint64_t> P((size_t)p.ncls << tp.n_held), count((size_t)p.ncls), A((size_t)1 << p.width), D((size_t)ttp.n_forget * (size_t)host_words_per_forget(p.width));
    for (uint64_t s = 0; s < N; ++s) {
        if (s == 0 || cq_rows != 1) site_cost_words(cq + (cq_rows == 1 ? 0u : s) * row, 1, p.nq, cw.data());
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        tiled_partials_fold(tp, reps.data(), threads, P.data(), cost.data(), count.data(),
                            [&](const uint32_t *rep, uint64_t *Amine) { return minplus_one_wide_site(tp, rep, cw.data(), Amine); });
        tiled_trace_classes(ttp, reps.data(), P.data(), A.data(), D.data(), chain_out + s * (uint64_t)p.ncls * (uint64_t)p.nq, [&](const uint32_t *rep, uint64_t *Am, uint64_t *Dm) {
            minplus_one_wide_traced(tp, rep, [&](uint64_t e, uint32_t q, uint32_t idx) { return e + ((uint64_t)site_cost(cw[q], idx) << kCountBits); }, Am, Dm);
        });
        for (int c = 0; c < p.ncls; ++c) {
            if (cost_out) cost_out[s * (uint64_t)p.ncls + c] = cost[(size_t)c];
            if (count_out) count_out[s * (uint64_t)p.ncls + c] = count[(size_t)c];
        }
    }
}

}  // namespace minplus

// class_minplus_tiled_trace.hip: all pointers are device pointers.  dev_ops, held, reps as class_minplus_tiled.hip takes them; wide_ops
// uint32[n_ops][kTiledOpWords]; pick uint32[S * ncls] (launch_minplus_pick); forget_tile uint32[n_forget][kForgetTileWords]; forget_words
// uint32[n_forget][W]; work uint64[pairs][2^state_bits] and D uint64[pairs][words_per_pair]: the state vectors and the decisions of one trace pass,
// both dirty; cw as the site sweep's; chain_out uint8[S * ncls][nq]: rows pair_first .. pair_first + pairs are overwritten.
struct MinplusTiledTraceArgs {
    uint32_t unit_first, units;        // the pairs syndrome * ncls + class of this pass, counted within the launch group
    int W, n_held, state_bits, tile_width;
    uint32_t op_first, op_count, tile, fixed_live, local_in, local_out, n_tiles, first, last;
    uint32_t forget_first, n_forget, words_per_tile;   // the ordinal of the segment's first FORGET
    uint32_t words_per_pair;
    uint32_t cxz[4];
    int ncls, nq, per_syndrome;        // the site kernel's (cxz is the uniform kernel's)
};
struct MinplusTiledWalkArgs {
    uint32_t pair_first, pairs;
    int W, n_held, n_ops, n_forget, nq;
    uint32_t words_per_tile, words_per_pair;
};
// the trace kernels of one pass, segment by segment, then k_minplus_tiled_walk: stream order is the only synchronisation.  cw == nullptr: the four
// costs cxz; otherwise the cost words
hipError_t launch_minplus_tiled_trace(const minplus::TiledTracePlan &ttp, const uint32_t *cxz, int per_syndrome, uint32_t pair_first, uint32_t pairs, const uint32_t *dev_ops,
                                      const uint32_t *wide_ops, const uint32_t *held, const uint32_t *reps, const uint32_t *cw, const uint32_t *pick, const uint32_t *forget_tile,
                                      const uint32_t *forget_words, uint64_t *work, uint64_t *D, uint8_t *chain_out, hipStream_t stream);

#ifdef __HIPCC__
namespace minplus {

// One workgroup of a tiled trace kernel, live tile blockIdx.x of pair a.unit_first + blockIdx.y under hbits = pick[pair]: sweep::tile_sweep's gather
// and write-back around the CLOSE and INTRO passes of class_sweep_ops.hpp and a FORGET that ballots.  The FORGET walks its local h in whole waves --
// the bound is wave-uniform, a lane past it or on a dead f stays in the wave and contributes 0; the LDS accesses stay behind the live mask -- and the
// wave's first lane stores __ballot(take) with one 64-bit vector store.  The last segment stores nothing: the partials are the sweep's.
template <class Args, class Src>
__device__ __forceinline__ void tile_sweep_traced(uint64_t *lds, const Args &a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                                  const uint32_t *__restrict__ reps, const uint32_t *__restrict__ pick, const uint32_t *__restrict__ forget_tile,
                                                  uint64_t *__restrict__ work, uint64_t *__restrict__ D, const Src &src)
{
    const uint32_t tid = threadIdx.x, threads = blockDim.x, lane = tid & (kTraceWave - 1u), pair = a.unit_first + blockIdx.y;
    const uint32_t hbits = pick[pair] & ((1u << a.n_held) - 1u);
    const uint32_t base = sweep::bits_deposit(blockIdx.x, a.fixed_live), entries = 1u << a.tile_width;
    uint64_t *A = work + ((size_t)blockIdx.y << a.state_bits) + base;
    uint64_t *mine = D + (size_t)blockIdx.y * (size_t)a.words_per_pair + (size_t)blockIdx.x * (size_t)a.words_per_tile;
    const uint32_t f0 = sweep::bits_deposit(tid, a.tile), step = sweep::bits_deposit(threads, a.tile);
    if (a.first) {
        if (tid == 0) lds[0] = 1ull;                                            // (0, 1)
    } else {
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_in)) lds[l] = A[f];
    }
    __syncthreads();
    const sweep::TileRep rep{sweep::HeldRep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W}, base};
    uint32_t fi = a.forget_first;
    for (uint32_t o = a.op_first; o < a.op_first + a.op_count; ++o) {
        const sweep::Op<sweep::TileOps> op(ops, o);
        if (op.kind == sweep::kClose) sweep::close_pass<MinPlus>(lds, tid, threads, op, rep, src);
        else if (op.kind == sweep::kIntro) sweep::intro_pass<MinPlus>(lds, tid, threads, op);
        else {
            const uint32_t n_h = 1u << (op.top - 1u), bit = 1u << op.slot;
            if (fi < a.n_forget) {                            // (always: the plan counts its FORGETs; a stream that does not cannot leave its rows of D)
                uint64_t *words = mine + forget_tile[kForgetTileWords * fi + 3u];
                for (uint32_t h0 = tid - lane; h0 < n_h; h0 += threads) {         // whole waves: h0 is wave-uniform
                    const uint32_t h = h0 + lane, f = sweep::insert_zero(h, op.slot);
                    const bool live = h < n_h && !(f & ~op.mask);
                    bool take = false;
                    if (live) {
                        const uint64_t off = lds[f], on = lds[f | bit];
                        take = (on >> kCountBits) < (off >> kCountBits);         // strict: a tie leaves the generator off
                        lds[f] = mp_combine(off, on);
                    }
                    const uint64_t word = __ballot(take);
                    if (lane == 0) words[h0 >> 6] = word;
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

}  // namespace minplus
#endif  // __HIPCC__

}  // namespace qecmc
