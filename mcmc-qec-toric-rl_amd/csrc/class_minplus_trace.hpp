// A shortest chain of every class: the (min, +) sweep of class_minplus.hpp traced back.  The sweep is integer, so which branch won at every FORGET is
// a function of exact values, and a tie rule makes the traced chain a pure function of (plan, representative, costs): the kernels
// (class_minplus_trace.hip) equal the twin byte for byte, whatever their order.  Counts play no part: a class whose count saturated still gets an
// exact chain.
//
// For one (syndrome, class) pair, with cut plan cp and class representative rep:
//     1. PARTIALS   P[h] = minplus_one under every assignment h of the held generators, as minplus_cut_host forms them.
//     2. PICK       h* = the lowest h whose P[h] has the least cost.  Only costs are compared.
//     3. FORWARD    the op loop of minplus_one under h*; at every FORGET one bit per live f with the slot bit clear,
//                       take = cost(A[f | bit]) < cost(A[f])            -- strict: a tie leaves the generator off --
//                   kept at (fi, h): fi the FORGET's ordinal in the stream, h the compressed index, f = insert_zero(h, slot).
//     4. WALK       f = 0, chain = cut_representative(cp, rep, h*); through the ops in reverse: FORGET: where bit (fi, remove_bit(f, slot)) is set,
//                   f |= bit and chain ^= forget_words[fi]; INTRO: f &= ~bit; CLOSE: nothing.  The walk ends at f == 0.
//     5. RESULT     the chain as bytes uint8[nq]; a cell no generator touches keeps the representative's byte.
//
// What the chain promises: it has the input's syndrome, it lies in class c, its cost is the sweep's cost_out, and it depends on (plan,
// representative, costs) alone.  Where count_out == 1 it is THE shortest chain of the class and so a function of the syndrome alone; where several
// chains tie it is the one the rule above selects from this representative -- another representative of the same syndrome may select another.
//
// THE DECISIONS of one pair are n_forget * words_per_forget 64-bit words, words_per_forget = max(1, 2^(width - 1) / 64): bit h of FORGET fi is bit
// h & 63 of word fi * words_per_forget + (h >> 6).  A FORGET writes every word its h reach (dead f write 0), the walk reads only bits of live f, so a
// dirty workspace is allowed.  120 KiB per pair at rotated L = 11; trace_launch_group bounds a launch group's workspace by kTraceWorkspaceBytes.
#pragma once
#include "class_minplus.hpp"

namespace qecmc {
namespace minplus {

constexpr uint64_t kTraceWorkspaceBytes = 256ull << 20;      // the decision words of one launch group

struct TracePlan {
    sweep::CutPlan cut;                 // refusal: cut.plan.refusal, prefixed "qecmc_class_minplus_chains:"
    int n_forget = 0, words_per_forget = 1;
    std::vector<int> forget_gen;        // [n_forget]: the table index of the generator FORGET fi retires, in stream order
    std::vector<uint32_t> forget_words; // [n_forget][W]: that generator as packed state words, 2 bits per qubit (held_words' layout)
};

// a refusal of the min-plus sweep under this entry point's name
inline Refusal chains_prefix(Refusal r)
{
    static const std::string from = "qecmc_class_minplus:";
    if (r.code && r.msg.compare(0, from.size(), from) == 0) r.msg = "qecmc_class_minplus_chains:" + r.msg.substr(from.size());
    return r;
}

inline Refusal check_chain_costs(const uint32_t *cost) { return chains_prefix(check_costs(cost)); }

constexpr int trace_words_per_forget(int width) { return width - 1 > 6 ? 1 << (width - 1 - 6) : 1; }

// the index f without its bit `slot`: the inverse of insert_zero on the f whose bit is clear
__host__ __device__ inline uint32_t remove_bit(uint32_t f, uint32_t slot) { return ((f >> (slot + 1u)) << slot) | (f & ((1u << slot) - 1u)); }

// the generator every FORGET of a cut plan's stream retires: Trace::forget_at of the final stream, in stream order -> forget_gen [n_forget] and
// forget_words [n_forget][W]; false where the stream does not retire every generator that is not held exactly once.  The (min, +) traceback and the
// exact sampler (class_sample.hpp) both walk their sweep back through these.
inline bool forget_generators(const sweep::CutPlan &cut, int code, int L, std::vector<int> &forget_gen, std::vector<uint32_t> &forget_words)
{
    const sweep::Plan &p = cut.plan;
    std::vector<char> held((size_t)p.n_gen, 0);
    for (const int g : cut.held) held[(size_t)g] = 1;
    sweep::Trace tr;
    const sweep::Stream st = sweep::build_stream(code, L, held, &tr);
    const correct::Table &ct = st.table;
    std::vector<int> at_op((size_t)p.n_ops, -1);                                // the generator forgotten at op o
    bool ok = st.head.refusal.code == 0 && (int)st.ops.size() == p.n_ops;
    for (int g = 0; ok && g < p.n_gen; ++g) {
        const int at = tr.forget_at[(size_t)g];
        if (held[(size_t)g]) { ok = at < 0; continue; }
        ok = at >= 0 && at < p.n_ops && at_op[(size_t)at] < 0 && (p.ops[(size_t)at * sweep::kOpWords] & 15u) == sweep::kForget;
        if (ok) at_op[(size_t)at] = g;
    }
    for (int o = 0; ok && o < p.n_ops; ++o) {
        if ((p.ops[(size_t)o * sweep::kOpWords] & 15u) != sweep::kForget) continue;
        const int g = at_op[(size_t)o];
        if (g < 0) { ok = false; break; }
        forget_gen.push_back(g);
        std::vector<uint32_t> words((size_t)ct.W, 0u);
        for (int i = 0; i < 4; ++i) {
            const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
            words[site >> 4] ^= pauli << ((site & 15u) * 2u);                   // (Pauli values XOR as the Pauli product)
        }
        forget_words.insert(forget_words.end(), words.begin(), words.end());
    }
    return ok && (int)forget_gen.size() == p.n_gen - cut.n_held;
}

// build_minplus_plan, its refusals renamed, and the generator every FORGET retires
inline TracePlan build_trace_plan(int code, int L, int lds_width)
{
    TracePlan tp;
    tp.cut = build_minplus_plan(code, L, lds_width);
    sweep::Plan &p = tp.cut.plan;
    if (p.refusal.code) { p.refusal = chains_prefix(p.refusal); return tp; }
    const bool ok = forget_generators(tp.cut, code, L, tp.forget_gen, tp.forget_words);
    tp.n_forget = (int)tp.forget_gen.size();
    tp.words_per_forget = trace_words_per_forget(p.width);
    if (!ok)
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_chains: internal: the stream of code %d at L=%d does not retire every generator once", code, L);
    return tp;
}

// the decision words of one (syndrome, class) pair, in bytes
inline uint64_t trace_bytes_per_pair(const TracePlan &tp) { return (uint64_t)tp.n_forget * (uint64_t)tp.words_per_forget * 8ull; }

// cut_launch_group, further bounded so that the decision words of one group -- group * ncls * bytes_per_pair -- stay within kTraceWorkspaceBytes;
// never 0: one syndrome is always launched
inline uint32_t trace_launch_group(uint64_t N, int ncls, int n_held, uint64_t bytes_per_pair)
{
    uint32_t group = sweep::cut_launch_group(N, ncls, n_held);
    const uint64_t per = (uint64_t)ncls * (bytes_per_pair ? bytes_per_pair : 1ull);
    const uint64_t cap = kTraceWorkspaceBytes / per;
    if (cap < group) group = cap < 1ull ? 1u : (uint32_t)cap;
    return group;
}

// step 2: the lowest h whose partial has the least cost
inline uint32_t pick_assignment(const uint64_t *P, int n_held)
{
    uint32_t best = 0;
    for (uint32_t h = 1; h < (1u << n_held); ++h)
        if ((P[h] >> kCountBits) < (P[best] >> kCountBits)) best = h;
    return best;
}

// step 3: which branch won at every FORGET of host_ops -- the strict rule, a tie leaves the generator off; a dead f leaves a 0, as the kernel's
// ballot does
struct Decisions {
    uint64_t *D;
    int words_per_forget, fi = 0;
    uint64_t *mine = nullptr;
    void begin(uint32_t n_h)
    {
        mine = D + (size_t)fi * (size_t)words_per_forget;
        for (uint32_t w = 0; w < (n_h + 63u) / 64u; ++w) mine[w] = 0ull;
    }
    void at(uint32_t h, uint64_t off, uint64_t on)
    {
        if ((on >> kCountBits) < (off >> kCountBits)) mine[h >> 6] |= 1ull << (h & 63u);
    }
    void end() { ++fi; }
};

// minplus_one with decisions.  A: 2^width entries of scratch, D: n_forget * words_per_forget words, both dirty allowed -> the packed partial
inline uint64_t minplus_one_traced(const TracePlan &tp, const uint32_t *rep, const uint32_t *cxz, uint64_t *A, uint64_t *D)
{
    const sweep::Plan &p = tp.cut.plan;
    A[0] = 1ull;
    sweep::host_ops(p.ops.data(), p.n_ops, rep, A, [&](uint64_t a, uint32_t, uint32_t idx) { return a + ((uint64_t)cxz[idx] << kCountBits); }, mp_combine,
                    Decisions{D, tp.words_per_forget});
    return A[0];
}

// step 4: the walk.  chain: W packed words, cut_representative(cp, rep, h*) on entry, the traced chain on return -> the f the walk ends at (0)
inline uint32_t trace_walk(const TracePlan &tp, const uint64_t *D, uint32_t *chain)
{
    using namespace sweep;
    const Plan &p = tp.cut.plan;
    uint32_t f = 0;
    int fi = tp.n_forget;
    for (int o = p.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = p.ops[(size_t)o * kOpWords], kind = w0 & 15u, slot = (w0 >> 4) & 15u, bit = 1u << slot;
        if (kind == kIntro) f &= ~bit;
        else if (kind == kForget) {
            --fi;
            const uint32_t h = remove_bit(f, slot);
            if ((D[(size_t)fi * (size_t)tp.words_per_forget + (h >> 6)] >> (h & 63u)) & 1ull) {
                f |= bit;
                for (int w = 0; w < p.W; ++w) chain[w] ^= tp.forget_words[(size_t)fi * p.W + w];
            }
        }
    }
    return f;
}

// step 5: packed words -> bytes
inline void unpack_chain(const uint32_t *words, int nq, uint8_t *out)
{
    for (int q = 0; q < nq; ++q) out[q] = (uint8_t)((words[q >> 4] >> ((q & 15) * 2)) & 3u);
}

// The twin.  chains uint8[N][nq], cost4[4] (I, X, Y, Z) -> chain_out uint8[N][ncls][nq]; cost_out uint32[N][ncls], count_out uint64[N][ncls] and
// cls int32[N] (all three nullable): minplus_cut_host's, exactly.  Threaded as minplus_cut_host: the partials of one syndrome are spread over
// `threads` host threads; the trace of a pair is one more pass and runs on the calling thread.
inline void minplus_trace_host(const TracePlan &tp, uint64_t N, const uint8_t *chains, const uint32_t *cost4, uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out,
                               int32_t *cls, unsigned threads = 0)
{
    const sweep::CutPlan &cp = tp.cut;
    const sweep::Plan &p = cp.plan;
    uint32_t cxz[4];
    costs_xz(cost4, cxz);
    const uint32_t n_h = 1u << cp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = sweep::host_threads(threads, n_work, n_work, cp.n_held == 0);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W);
    std::vector<uint64_t> P((size_t)n_work), A((size_t)1 << p.width), D((size_t)tp.n_forget * (size_t)tp.words_per_forget);
    for (uint64_t s = 0; s < N; ++s) {
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        sweep::host_partials(n_work, threads, p.width, p.W, P.data(), [&](uint32_t i, uint32_t *mine, uint64_t *Amine) {
            sweep::cut_representative(cp, &reps[(size_t)(i >> cp.n_held) * p.W], i & (n_h - 1u), mine);
            return minplus_one(p, mine, cxz, Amine);
        });
        for (int c = 0; c < p.ncls; ++c) {
            const uint64_t *mine = &P[(size_t)c << cp.n_held];
            const uint32_t pick = pick_assignment(mine, cp.n_held);
            sweep::cut_representative(cp, &reps[(size_t)c * p.W], pick, rep.data());
            minplus_one_traced(tp, rep.data(), cxz, A.data(), D.data());
            trace_walk(tp, D.data(), rep.data());
            unpack_chain(rep.data(), p.nq, chain_out + (s * (uint64_t)p.ncls + (uint64_t)c) * (uint64_t)p.nq);
            uint64_t e = mine[0];
            for (uint32_t h = 1; h < n_h; ++h) e = mp_combine(e, mine[h]);
            uint32_t cost;
            uint64_t count;
            mp_unpack(e, p.n_gen - p.rank, &cost, &count);
            if (cost_out) cost_out[s * (uint64_t)p.ncls + c] = cost;
            if (count_out) count_out[s * (uint64_t)p.ncls + c] = count;
        }
    }
}

}  // namespace minplus

#ifdef __HIPCC__
namespace minplus {
constexpr uint32_t kTraceWave = 64;

// One workgroup of a trace kernel (k_minplus_trace, k_minplus_trace_site), pair blockIdx.x under hbits = pick[pair]: the CLOSE and INTRO passes of
// class_sweep_ops.hpp in the algebra MinPlus, and a FORGET that walks its h in whole waves -- the loop bound is wave-uniform, a lane past the bound
// or on a dead f stays in the wave and contributes 0 -- so that __ballot(live && take) is the 64 decisions of h0 .. h0 + 63; the first lane of the
// wave stores it to D[pair][fi][h0 >> 6] with one 64-bit vector store.  Where 2^(top - 1) < 64 the one word is word 0 of wave 0.  The LDS accesses
// stay behind the live mask.  src: the costs of a CLOSE.
template <class TraceArgs, class Src>
__device__ __forceinline__ void trace_sweep(uint64_t *A, const TraceArgs &t, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                            const uint32_t *__restrict__ reps, const uint32_t *__restrict__ pick, uint64_t *__restrict__ D, const Src &src)
{
    const auto &a = t.m;
    const uint32_t tid = threadIdx.x, threads = blockDim.x, lane = tid & (kTraceWave - 1u), pair = blockIdx.x, hbits = pick[pair] & ((1u << a.n_held) - 1u);
    const sweep::HeldRep rep{reps + (size_t)pair * (size_t)a.W, held, hbits, (uint32_t)a.W};
    uint64_t *mine = D + (size_t)pair * (size_t)t.n_forget * (size_t)t.words_per_forget;
    int fi = 0;
    if (tid == 0) A[0] = 1ull;                                // (0, 1)
    __syncthreads();
    for (uint32_t o = 0; o < (uint32_t)a.n_ops; ++o) {
        const sweep::Op<sweep::NarrowOps> op(ops, o);
        if (op.kind == sweep::kClose) sweep::close_pass<MinPlus>(A, tid, threads, op, rep, src);
        else if (op.kind == sweep::kIntro) sweep::intro_pass<MinPlus>(A, tid, threads, op);
        else {
            const uint32_t n_h = 1u << (op.top - 1u), bit = 1u << op.slot;
            if (fi < t.n_forget)                              // (always: the plan counts its FORGETs; a stream that does not cannot leave its rows of D)
                for (uint32_t h0 = tid - lane; h0 < n_h; h0 += threads) {          // whole waves: h0 is wave-uniform
                    const uint32_t h = h0 + lane, f = sweep::insert_zero(h, op.slot);
                    const bool live = h < n_h && !(f & ~op.mask);
                    bool take = false;
                    if (live) {
                        const uint64_t off = A[f], on = A[f | bit];
                        take = (on >> kCountBits) < (off >> kCountBits);           // strict: a tie leaves the generator off
                        A[f] = mp_combine(off, on);
                    }
                    const uint64_t word = __ballot(take);
                    if (lane == 0) mine[(size_t)fi * (size_t)t.words_per_forget + (h0 >> 6)] = word;
                }
            ++fi;
        }
        __syncthreads();
    }
}
}  // namespace minplus
#endif

// class_minplus_trace.hip: all pointers are device pointers.  ops, held, reps and P as class_minplus.hip takes them; pick uint32[S * ncls];
// D uint64[S * ncls][n_forget][words_per_forget]: scratch, dirty allowed; forget_words uint32[n_forget][W]; chain_out uint8[S * ncls][nq]: overwritten.
struct MinplusTraceArgs {
    MinplusArgs m;
    int n_forget, words_per_forget, nq;
};
hipError_t class_minplus_trace_allow_lds(int width);   // hipSuccess: k_minplus_trace can be launched with a state vector of this width on the current device
// between launch_class_minplus_sweep and launch_class_minplus_reduce, on their stream: the reduce destroys the partials
hipError_t launch_minplus_pick(const MinplusArgs &a, const uint64_t *P, uint32_t *pick, hipStream_t stream);
// k_minplus_walk alone, after a kernel that wrote the decision words D on the same stream (launch_minplus_trace ends with it; class_minplus_site.hip
// runs it after its own trace kernel): the walk looks at no cost
hipError_t launch_minplus_walk(const MinplusTraceArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *forget_words, const uint32_t *pick,
                               const uint64_t *D, uint8_t *chain_out, hipStream_t stream);
// k_minplus_trace, then k_minplus_walk: stream order is the only synchronisation
hipError_t launch_minplus_trace(const MinplusTraceArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *forget_words, const uint32_t *pick,
                                uint64_t *D, uint8_t *chain_out, hipStream_t stream);

}  // namespace qecmc
