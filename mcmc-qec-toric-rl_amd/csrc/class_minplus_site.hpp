// The (min, +, count) sweep of class_minplus.hpp and its traceback (class_minplus_trace.hpp) under a cost per (syndrome, qubit): erasures -- an
// erased qubit costs nothing, whatever it carries --, inhomogeneous noise, soft priors put on an integer scale.  The plans, the op streams, the holds
// and the launch groups are the siblings', unchanged; a CLOSE names its qubit (op[3]), and the one difference is that the cost it adds comes from a
// table row instead of four numbers shared by all qubits -- what class_sweep_site.hpp does on the sum-product side.
//
// THE TABLE.  The caller's cq is uint8[cq_rows][nq][4], the costs of I, X, Y, Z at every cell of the state layout; cq_rows is 1 -- one table for
// every syndrome -- or N -- row s belongs to syndrome s.  Host and device read it as one uint32 per qubit, the four bytes in (x, z) order I, X, Z, Y
// (site_cost_words), as the siblings read their four costs: the cost of idx is (word >> 8 * idx) & 255.  The word of the CLOSE of qubit q in
// syndrome s is at (per_syndrome ? s : 0) * nq + q.  The device holds the rows of one launch group at a time (s counts within the group), or the one
// table once: nothing grows with N.
//
// COSTS.  Every byte value is a cost: 0 .. 255, zero allowed anywhere, a non-zero cost of I as well.  check_cost_range holds at every accepted
// shape, so the 16 bits of an entry's cost never wrap.  Only the words of qubits some CLOSE names are read (sweep::closed_qubits): a cell that holds
// no qubit (the planar code's unused cells) may hold anything.
//
// ARITHMETIC.  minplus_one_site, minplus_cut_site_host, minplus_one_traced_site and minplus_trace_site_host are minplus_one, minplus_cut_host,
// minplus_one_traced and minplus_trace_host entry for entry; pick_assignment, trace_walk, unpack_chain, mp_combine, mp_unpack, the count shift and
// the saturation are those.  Integer throughout: each twin equals its kernel (class_minplus_site.hip) exactly, and with constant rows its uniform
// sibling, chains included.
//
// Refused, before a device is looked for: what build_minplus_plan / build_trace_plan refuse, with their codes, the message prefixed
// "qecmc_class_minplus_site:" / "qecmc_class_minplus_chains_site:"; QECMC_ERR_INVALID for a NULL table and for a cq_rows that is neither 1 nor N
// (N > 0).
#pragma once
#include "class_minplus_trace.hpp"
#include "class_sweep_site.hpp"

namespace qecmc {
namespace minplus {

// a refusal of the uniform entry point `from` ("qecmc_class_minplus:" / "qecmc_class_minplus_chains:") under the site entry point's name
inline Refusal site_prefix(Refusal r, const char *from, const char *to)
{
    const std::string f(from);
    if (r.code && r.msg.compare(0, f.size(), f) == 0) r.msg = std::string(to) + r.msg.substr(f.size());
    return r;
}

inline sweep::CutPlan build_minplus_site_plan(int code, int L, int lds_width)
{
    sweep::CutPlan cp = build_minplus_plan(code, L, lds_width);
    cp.plan.refusal = site_prefix(cp.plan.refusal, "qecmc_class_minplus:", "qecmc_class_minplus_site:");
    return cp;
}

inline TracePlan build_trace_site_plan(int code, int L, int lds_width)
{
    TracePlan tp = build_trace_plan(code, L, lds_width);
    tp.cut.plan.refusal = site_prefix(tp.cut.plan.refusal, "qecmc_class_minplus_chains:", "qecmc_class_minplus_chains_site:");
    return tp;
}

// check_site_rows (class_sweep_site.hpp) for the cost table, under the entry point's name
inline Refusal check_cost_rows(const char *entry, uint64_t N, uint64_t cq_rows)
{
    if (N > 0 && cq_rows != 1 && cq_rows != N)
        return refuse_params(QECMC_ERR_INVALID, "%s: cq_rows=%llu: the site costs are one table (1) or one per syndrome (N=%llu)", entry, (unsigned long long)cq_rows,
                             (unsigned long long)N);
    return {};
}

// rows of cq as words: out uint32[rows][nq], the bytes of a word in (x, z) order I, X, Z, Y (costs_xz per qubit; cells that hold no qubit are
// packed as they are)
inline void site_cost_words(const uint8_t *cq, uint64_t rows, int nq, uint32_t *out)
{
    for (uint64_t i = 0; i < rows * (uint64_t)nq; ++i) {
        const uint8_t *c = cq + i * 4u;
        out[i] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[3] << 16) | ((uint32_t)c[2] << 24);
    }
}

// the cost of idx (x | z << 1) in a qubit's word
__host__ __device__ inline uint32_t site_cost(uint32_t word, uint32_t idx) { return (word >> (8u * idx)) & 255u; }

// minplus_one() with the cost word of the CLOSE's qubit: cw uint32[nq]
inline uint64_t minplus_one_site(const sweep::Plan &p, const uint32_t *rep, const uint32_t *cw, uint64_t *A)
{
    A[0] = 1ull;                                                                // (0, 1)
    sweep::host_ops(p.ops.data(), p.n_ops, rep, A, [&](uint64_t a, uint32_t q, uint32_t idx) { return a + ((uint64_t)site_cost(cw[q], idx) << kCountBits); }, mp_combine,
                    sweep::NoDecisions{});
    return A[0];
}

// minplus_one_traced() with the cost word of the CLOSE's qubit
inline uint64_t minplus_one_traced_site(const TracePlan &tp, const uint32_t *rep, const uint32_t *cw, uint64_t *A, uint64_t *D)
{
    const sweep::Plan &p = tp.cut.plan;
    A[0] = 1ull;
    sweep::host_ops(p.ops.data(), p.n_ops, rep, A, [&](uint64_t a, uint32_t q, uint32_t idx) { return a + ((uint64_t)site_cost(cw[q], idx) << kCountBits); }, mp_combine,
                    Decisions{D, tp.words_per_forget});
    return A[0];
}

// the partials of one syndrome under its cost words, spread over host threads as minplus_cut_host spreads them
inline void site_cost_partials(const sweep::CutPlan &cp, const uint32_t *reps, const uint32_t *cw, unsigned threads, uint64_t *P)
{
    const sweep::Plan &p = cp.plan;
    const uint32_t n_h = 1u << cp.n_held, n_work = (uint32_t)p.ncls * n_h;
    sweep::host_partials(n_work, sweep::host_threads(threads, n_work, n_work, cp.n_held == 0), p.width, p.W, P, [&](uint32_t i, uint32_t *rep, uint64_t *A) {
        sweep::cut_representative(cp, &reps[(size_t)(i >> cp.n_held) * p.W], i & (n_h - 1u), rep);
        return minplus_one_site(p, rep, cw, A);
    });
}

// The twin of qecmc_class_minplus_site.  chains uint8[N][nq], cq uint8[cq_rows][nq][4] (I, X, Y, Z), cq_rows 1 or N -> cost_out uint32[N][ncls],
// count_out uint64[N][ncls]; cls int32[N] (nullable).
inline void minplus_cut_site_host(const sweep::CutPlan &cp, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, uint32_t *cost_out, uint64_t *count_out,
                                  int32_t *cls, unsigned threads = 0)
{
    const sweep::Plan &p = cp.plan;
    const uint32_t n_h = 1u << cp.n_held;
    const size_t row = (size_t)p.nq * 4u;
    std::vector<uint32_t> cw((size_t)p.nq), reps((size_t)p.ncls * p.W);
    std::vector<uint64_t> P((size_t)p.ncls * n_h);
    for (uint64_t s = 0; s < N; ++s) {
        if (s == 0 || cq_rows != 1) site_cost_words(cq + (cq_rows == 1 ? 0u : s) * row, 1, p.nq, cw.data());
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        site_cost_partials(cp, reps.data(), cw.data(), threads, P.data());
        for (int c = 0; c < p.ncls; ++c) {
            uint64_t e = P[(size_t)c << cp.n_held];
            for (uint32_t h = 1; h < n_h; ++h) e = mp_combine(e, P[((size_t)c << cp.n_held) + h]);
            mp_unpack(e, p.n_gen - p.rank, &cost_out[s * (uint64_t)p.ncls + c], &count_out[s * (uint64_t)p.ncls + c]);
        }
    }
}

// The twin of qecmc_class_minplus_chains_site.  As minplus_cut_site_host, and chain_out uint8[N][ncls][nq]; cost_out, count_out and cls nullable.
inline void minplus_trace_site_host(const TracePlan &tp, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, uint8_t *chain_out, uint32_t *cost_out,
                                    uint64_t *count_out, int32_t *cls, unsigned threads = 0)
{
    const sweep::CutPlan &cp = tp.cut;
    const sweep::Plan &p = cp.plan;
    const uint32_t n_h = 1u << cp.n_held;
    const size_t row = (size_t)p.nq * 4u;
    std::vector<uint32_t> cw((size_t)p.nq), reps((size_t)p.ncls * p.W), rep((size_t)p.W);
    std::vector<uint64_t> P((size_t)p.ncls * n_h), A((size_t)1 << p.width), D((size_t)tp.n_forget * (size_t)tp.words_per_forget);
    for (uint64_t s = 0; s < N; ++s) {
        if (s == 0 || cq_rows != 1) site_cost_words(cq + (cq_rows == 1 ? 0u : s) * row, 1, p.nq, cw.data());
        const int a = sweep::class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        site_cost_partials(cp, reps.data(), cw.data(), threads, P.data());
        for (int c = 0; c < p.ncls; ++c) {
            const uint64_t *mine = &P[(size_t)c << cp.n_held];
            const uint32_t pick = pick_assignment(mine, cp.n_held);
            sweep::cut_representative(cp, &reps[(size_t)c * p.W], pick, rep.data());
            minplus_one_traced_site(tp, rep.data(), cw.data(), A.data(), D.data());
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

#ifdef __HIPCC__
// the factor source of a CLOSE: the cost word of its qubit, one wave-uniform scalar load; the cost of idx is a shift by 8 * idx and a mask
struct SiteCosts {
    const uint32_t *words;
    struct Word {
        uint32_t word;
        __device__ __forceinline__ uint32_t at(uint32_t idx) const { return site_cost(word, idx); }
    };
    __device__ __forceinline__ Word row(uint32_t q) const { return {words[q]}; }
};
#endif

}  // namespace minplus

// class_minplus_site.hip: all pointers are device pointers, as the siblings take them; cw uint32[per_syndrome ? S : 1][t.nq], a word per qubit in
// (x, z) byte order.  S counts the syndromes of the launch group and the rows of cw with it.  t.m.cxz is not read.
struct MinplusSiteArgs {
    MinplusTraceArgs t;                                // the sweep kernel reads t.m and t.nq; the trace kernel all of it
    int per_syndrome;
};
hipError_t class_minplus_site_allow_lds(int width);          // class_minplus_allow_lds() for k_class_minplus_site
hipError_t class_minplus_trace_site_allow_lds(int width);    // class_minplus_trace_allow_lds() for k_minplus_trace_site
// k_class_minplus_site alone: launch_class_minplus_reduce (and launch_minplus_pick before it) follow on the same stream
hipError_t launch_class_minplus_site_sweep(const MinplusSiteArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *cw, uint64_t *P,
                                           hipStream_t stream);
// k_minplus_trace_site alone: launch_minplus_walk follows on the same stream
hipError_t launch_minplus_trace_site(const MinplusSiteArgs &a, const uint32_t *ops, const uint32_t *held, const uint32_t *reps, const uint32_t *cw, const uint32_t *pick,
                                     uint64_t *D, hipStream_t stream);

}  // namespace qecmc
