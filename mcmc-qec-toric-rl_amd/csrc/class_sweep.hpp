// The exact class law by a frontier sweep.  The weight of a chain is a product over qubits, so the class weight
//     Z_c = sum over s in {0,1}^G of prod_q w(P_q(s)),      P_q(s) = the representative of class c at q times the generators g with s_g = 1 that touch q,
// is the partition function of a model with local factors: every qubit is touched by at most four generators.  Variable elimination across the lattice
// needs (2 G + nq) 2^width operations instead of 2^G terms, `width` being the largest number of generators that are decided but still touch an
// undecided qubit.  The sum runs over the FULL generator table, dependent generators included: every group element is then met 2^(G - rank) times
// (4 on the torus, 1 elsewhere) and the result is multiplied by 2^-(G - rank), a power of two -- exact.
//
// THE PLAN (build_plan) is an op stream over `width` slots, the bit positions of the index f of a state vector A[2^width] of doubles, A[0] = 1 at first:
//     INTRO slot     A[f | 1 << slot] = A[f]                          for every live f with that bit clear: generator `slot` is now undecided-and-open
//     CLOSE qubit    A[f] *= w[chain_q (+) the Paulis whose slot bit is set in f]   for every live f; up to four (slot, Pauli) pairs, (+) on the (x, z) bits
//     FORGET slot    A[f] += A[f | 1 << slot]                         for every live f with that bit clear: the slot is free again
// and Z = A[0] * 2^-(G - rank) after the last op.  "Live f": no bit outside the op's mask of occupied slots; such entries are the only ones ever read,
// and every one of them was written before (an INTRO writes the entries it makes live), so the state vector needs no initialisation beyond A[0].
// The order is built from the supports: qubits in the row-major order of their cell on the lattice (cell_key: the one place that knows the geometry),
// each qubit's not-yet-introduced generators introduced just before it, a generator forgotten as soon as none of its qubits is open, the lowest free
// slot first.  A cell no generator touches (the planar code's unused cells) holds no qubit and is not in the stream.
//
// ARITHMETIC: every entry sees a fixed sequence of copies, single multiplies and single adds -- no reduction tree --, so the kernel (class_sweep.hip)
// and the twin (sweep_host) agree bit for bit, as long as neither contracts a multiply into an add: there is none to contract (every result goes
// through memory), and both are built with -ffp-contract=off.
//
// Refused, before a device is looked for: QECMC_ERR_INVALID for a (code, L) check_code_L() does not know; QECMC_ERR_UNSUPPORTED for a (code, L) without
// a class move (the toric code at even L) and for a plan wider than kMaxWidth -- what lds_carve(), which the launch calls too, fits into the LDS of
// one workgroup.  Accepted today: toric L = 3; planar L = 3 .. 6; xzzx / rotated L = 3, 5, 7, 9.  Width 14 (xzzx / rotated L = 11, planar L = 7) would
// need 128 KiB in place and is refused by name here; class_sweep_cut.hpp takes it, and the toric code at L = 5, through build_plan_held().
#pragma once
#include "../../include/qecmc.h"

#include <cmath>
#include <cstdint>
#include <vector>

#include "class_sweep_ops.hpp" // the op words, and the loop every twin and every kernel runs over them
#include "corrections.hpp"     // the class function on the packed state, the logical masks and the class-move table
#include "plan_host.hpp"       // Refusal, check_code_L

namespace qecmc {
namespace sweep {

constexpr int kThreads = 256;
constexpr uint32_t kGroupMax = 1024;         // syndromes of one launch: the device blocks hold kGroupMax * ncls * (W words + one double) at most, whatever N
constexpr uint32_t kLdsBudget = 64 * 1024;   // the default dynamic-LDS window: two workgroups of the widest plan fit the 160 KiB of a CU

// The LDS of one workgroup: the state vector alone, double[2^width], updated in place.
struct Carve {
    uint32_t entries = 0, bytes = 0;
};
constexpr Carve lds_carve(int width) { return width < 0 || width > 28 ? Carve{0u, 0u} : Carve{1u << width, 8u << width}; }
constexpr int max_width()
{
    int w = 0;
    while (lds_carve(w + 1).bytes != 0 && lds_carve(w + 1).bytes <= kLdsBudget) ++w;
    return w;
}
constexpr int kMaxWidth = max_width();       // 13
static_assert(kMaxWidth == 13 && kMaxWidth <= 16, "the op words keep a slot in 4 bits and the mask in 16");

struct Plan {
    int code = 0, L = 0, nq = 0, W = 0, ncls = 0, kinds = 0, n_gen = 0, rank = 0, width = 0, n_ops = 0, n_qubits = 0;
    double scale = 1.0;                // 2^-(n_gen - rank)
    std::vector<uint32_t> ops;         // [n_ops][kOpWords]
    std::vector<uint32_t> masks, need; // correct::Table's
    Carve carve;
    Refusal refusal;                   // code != 0: the (code, L) is refused; width and n_ops are still the planner's where it got that far
};

// the row-major key of a qubit's cell on the lattice, rows and columns in half steps: toric / planar layer 0 holds the vertical edges, layer 1 the
// horizontal ones (tables::toric_generator_table, surf_generator: the sites of a generator are the neighbours of its cell in these coordinates)
inline uint32_t cell_key(int code, int L, int q)
{
    const int LL = L * L, layer = q / LL, r = (q % LL) / L, c = q % L;
    if (code == QECMC_TORIC) return layer ? (uint32_t)((2 * r) * 2 * L + 2 * c + 1) : (uint32_t)((2 * r + 1) * 2 * L + 2 * c);
    if (code == QECMC_PLANAR) return layer ? (uint32_t)((2 * r + 1) * 2 * L + 2 * c + 1) : (uint32_t)((2 * r) * 2 * L + 2 * c);
    return (uint32_t)q;
}

// the rank of the generator table: greedy elimination in table order over the 2 nq-bit vectors (x bits, then z bits), as enumerate.hpp's basis
inline int generator_rank(const correct::Table &ct)
{
    const size_t nw = ((size_t)2 * ct.nq + 63) / 64;
    std::vector<std::vector<uint64_t>> rows;
    std::vector<size_t> pivot;
    for (int g = 0; g < ct.n_gen; ++g) {
        std::vector<uint64_t> v(nw, 0);
        for (int i = 0; i < 4; ++i) {
            const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
            if (pauli == 0u) continue;
            if (pauli == 1u || pauli == 2u) v[site >> 6] ^= 1ull << (site & 63);
            if (pauli >= 2u) v[((size_t)ct.nq + site) >> 6] ^= 1ull << (((size_t)ct.nq + site) & 63);
        }
        for (size_t i = 0; i < rows.size(); ++i)
            if ((v[pivot[i] >> 6] >> (pivot[i] & 63)) & 1u)
                for (size_t w = 0; w < nw; ++w) v[w] ^= rows[i][w];
        for (size_t b = 0; b < nw * 64; ++b)
            if ((v[b >> 6] >> (b & 63)) & 1u) { pivot.push_back(b); rows.push_back(v); break; }   // (its lowest set bit: no later row keeps it)
    }
    return (int)rows.size();
}

// What build_plan_held() saw on the way, for a planner that holds generators out (class_sweep_cut.hpp): where in the stream every generator is
// introduced and forgotten (-1: held, or never met), and the first op at which the number of live slots reaches its peak.
struct Trace {
    std::vector<int> intro_at, forget_at;
    int first_peak_op = -1;
};

// The op stream before it is encoded: what build_plan_held() and the wide encoder of class_sweep_tiled.hpp both read.  `live`: the occupied slots
// -- INTRO before it, CLOSE as they are, FORGET after it.  A pair is (slot, xz) of a generator's Pauli at the CLOSE's qubit.
struct StreamOp {
    uint32_t kind, slot, qubit, pairs, pair_slot[4], pair_xz[4];
    std::vector<char> live;
};
struct Stream {
    Plan head;                         // code .. n_ops and width, ops empty; refusal: not a (code, L), no class move, or an internal one
    std::vector<StreamOp> ops;
    int live_at_end = 0;
    correct::Table table;
};

// The stream of build_plan() with the generators g that have held[g] != 0 left out of the elimination: they get no INTRO and no FORGET and no CLOSE
// names them; a qubit they alone touch is still closed, with no pair.  `held` empty: nothing held.  Slots are handed out without a bound, so a
// refusal can name the width.
inline Stream build_stream(int code, int L, const std::vector<char> &held, Trace *trace)
{
    Stream st;
    Plan &p = st.head;
    p.code = code; p.L = L;
    if ((p.refusal = check_code_L(code, L)).code) return st;
    st.table = correct::build_table(code, L);
    const correct::Table &ct = st.table;
    p.nq = ct.nq; p.W = ct.W; p.ncls = ct.ncls; p.kinds = ct.kinds; p.n_gen = ct.n_gen;
    if (ct.need.empty()) {
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "no class move for code %d at L=%d: its logical operators do not reach every equivalence class (the toric code's "
                                                         "parity class does not see a logical line of even length)", code, L);
        return st;
    }
    // ---- the supports: which generators touch a qubit, with which Pauli; how many of a generator's qubits are still open
    struct Touch { int gen; uint32_t xz; };
    std::vector<std::vector<Touch>> touch((size_t)p.nq);
    std::vector<int> open((size_t)p.n_gen, 0);
    std::vector<char> is_qubit((size_t)p.nq, 0);
    for (int g = 0; g < p.n_gen; ++g)
        for (int i = 0; i < 4; ++i) {
            const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
            if (pauli == 0u) continue;
            if ((int)site >= p.nq) { p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: generator %d of code %d at L=%d leaves the state", g, code, L); return st; }
            is_qubit[site] = 1;
            if ((size_t)g < held.size() && held[(size_t)g]) continue;
            touch[site].push_back({g, pauli_to_xz(pauli)});
            ++open[(size_t)g];
        }
    std::vector<int> order;
    for (int q = 0; q < p.nq; ++q) {
        if (touch[(size_t)q].size() > 4) { p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: qubit %d of code %d at L=%d is touched by more than four generators", q, code, L); return st; }
        if (is_qubit[(size_t)q]) order.push_back(q);                            // (a cell no generator touches holds no qubit)
    }
    for (size_t i = 1; i < order.size(); ++i)                                   // insertion sort by the cell's key
        for (size_t j = i; j > 0 && cell_key(code, L, order[j - 1]) > cell_key(code, L, order[j]); --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    p.n_qubits = (int)order.size();
    // ---- the stream
    if (trace) { trace->intro_at.assign((size_t)p.n_gen, -1); trace->forget_at.assign((size_t)p.n_gen, -1); trace->first_peak_op = -1; }
    std::vector<int> slot_of((size_t)p.n_gen, -1);
    std::vector<char> used;
    std::vector<StreamOp> &stream = st.ops;
    int live = 0;
    for (const int q : order) {
        for (const Touch &t : touch[(size_t)q]) {
            if (slot_of[(size_t)t.gen] >= 0) continue;
            size_t s = 0;
            while (s < used.size() && used[s]) ++s;                             // the lowest free slot
            if (s == used.size()) used.push_back(0);
            if (trace) trace->intro_at[(size_t)t.gen] = (int)stream.size();
            stream.push_back({kIntro, (uint32_t)s, 0u, 0u, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, used});
            used[s] = 1; slot_of[(size_t)t.gen] = (int)s;
            if (++live > p.width) { p.width = live; if (trace) trace->first_peak_op = (int)stream.size() - 1; }
        }
        StreamOp close = {kClose, 0u, (uint32_t)q, 0u, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, used};
        for (const Touch &t : touch[(size_t)q]) { close.pair_slot[close.pairs] = (uint32_t)slot_of[(size_t)t.gen]; close.pair_xz[close.pairs++] = t.xz; }
        stream.push_back(close);
        for (const Touch &t : touch[(size_t)q]) {
            if (--open[(size_t)t.gen]) continue;
            const uint32_t s = (uint32_t)slot_of[(size_t)t.gen];
            used[s] = 0; --live;
            if (trace) trace->forget_at[(size_t)t.gen] = (int)stream.size();
            stream.push_back({kForget, s, 0u, 0u, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, used});
        }
    }
    p.n_ops = (int)stream.size();
    st.live_at_end = live;
    return st;
}

// what every encoder fills in after its op words: the rank and the scale, the class-move table, the LDS of a state vector of the plan's width
inline void finish_plan(Plan &p, const correct::Table &ct)
{
    p.rank = generator_rank(ct);
    p.scale = std::ldexp(1.0, -(p.n_gen - p.rank));
    p.masks = ct.masks; p.need = ct.need;
    p.carve = lds_carve(p.width);
}

// build_stream() in the four-word encoding above.  A plan wider than max_width is refused by name and not encoded.
inline Plan build_plan_held(int code, int L, const std::vector<char> &held, int max_width, Trace *trace)
{
    const Stream st = build_stream(code, L, held, trace);
    Plan p = st.head;
    if (p.refusal.code) return p;
    if (p.width > max_width) {
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "the frontier of code %d at L=%d is %d generators wide: a state vector of 2^%d doubles does not fit the %u bytes of "
                                                         "LDS a workgroup sweeps in (width %d at most)", code, L, p.width, p.width, lds_carve(max_width).bytes, max_width);
        return p;
    }
    if (st.live_at_end != 0) { p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: the plan of code %d at L=%d ends with %d live slots", code, L, st.live_at_end); return p; }
    for (const StreamOp &o : st.ops) {
        uint32_t mask = 0, top = 0, pair[4];
        for (size_t s = 0; s < o.live.size(); ++s)
            if (o.live[s]) mask |= 1u << s;
        const uint32_t reach = o.kind == kClose ? mask : mask | (1u << o.slot);
        while (top < 32u && (reach >> top)) ++top;
        if ((int)top > p.width || (int)o.qubit >= p.nq) { p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: an op of code %d at L=%d leaves its state vector", code, L); return p; }
        for (int j = 0; j < 4; ++j) pair[j] = (uint32_t)j < o.pairs ? (o.pair_slot[j] & 15u) | (o.pair_xz[j] << 4) : 0u;
        p.ops.push_back(o.kind | (o.slot << 4) | (o.pairs << 8) | (top << 12));
        p.ops.push_back(mask);
        p.ops.push_back(pair[0] | (pair[1] << 8) | (pair[2] << 16) | (pair[3] << 24));
        p.ops.push_back(o.qubit);
    }
    finish_plan(p, st.table);
    return p;
}

inline Plan build_plan(int code, int L) { return build_plan_held(code, L, {}, kMaxWidth, nullptr); }
static_assert(lds_carve(kMaxWidth).bytes == kLdsBudget, "build_plan's refusal names the budget");

// the four weights: finite and > 0
inline Refusal check_weights(const double *w)
{
    for (int i = 0; i < 4; ++i)
        if (!(w[i] > 0.0) || !std::isfinite(w[i]))
            return refuse_params(QECMC_ERR_INVALID, "w[%d]=%g: the weights of I, X, Y and Z are finite and > 0", i, w[i]);
    return {};
}

// one chain uint8[nq]: its class, and the representative of every class as packed state words -- reps uint32[ncls][W], 2 bits per qubit: the input
// times the kinds need[class of the input][c] names, at position 0 (enumr::class_representatives' rule)
inline int class_representatives(const Plan &p, const uint8_t *chain, uint32_t *reps)
{
    std::vector<uint32_t> words((size_t)p.W, 0u);
    for (int q = 0; q < p.nq; ++q) words[(size_t)(q >> 4)] |= (uint32_t)(chain[q] & 3u) << ((q & 15) * 2);
    lift::HostState st{words.data()};
    const int a = correct::class_of(st, p.code, p.L, p.W);
    for (int c = 0; c < p.ncls; ++c)
        for (int w = 0; w < p.W; ++w) {
            uint32_t v = words[(size_t)w];
            for (int kind = 0; kind < p.kinds; ++kind)
                if ((p.need[(size_t)a * p.ncls + c] >> kind) & 1u) v ^= p.masks[((size_t)kind * (p.L + 1)) * p.W + w];
            reps[(size_t)c * p.W + w] = v;
        }
    return a;
}

// the weight table in (x, z) order: I, X, Z, Y
inline void weights_xz(const double *w, double *wxz) { wxz[0] = w[0]; wxz[1] = w[1]; wxz[2] = w[3]; wxz[3] = w[2]; }

// one representative (packed words) through the op stream: the twin of one workgroup of class_sweep.hip.  A: 2^width doubles of scratch.
inline double sweep_one(const Plan &p, const uint32_t *rep, const double *wxz, double *A)
{
    A[0] = 1.0;
    host_ops(p.ops.data(), p.n_ops, rep, A, [&](double a, uint32_t, uint32_t idx) { return a * wxz[idx]; }, [](double a, double b) { return a + b; }, NoDecisions{});
    return A[0] * p.scale;
}

// The twin.  chains uint8[N][nq], w[4] (I, X, Y, Z) -> Z double[N][ncls]; cls int32[N] (nullable): the class of every input.
inline void sweep_host(const Plan &p, uint64_t N, const uint8_t *chains, const double *w, double *Z, int32_t *cls)
{
    double wxz[4];
    weights_xz(w, wxz);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    std::vector<double> A((size_t)1 << p.width);
    for (uint64_t s = 0; s < N; ++s) {
        const int a = class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        for (int c = 0; c < p.ncls; ++c) Z[s * (uint64_t)p.ncls + c] = sweep_one(p, &reps[(size_t)c * p.W], wxz, A.data());
    }
}

// How a batch becomes launches: groups of at most kGroupMax syndromes, one workgroup per (class, syndrome) of a group.
inline uint32_t launch_group(uint64_t N) { return N < kGroupMax ? (N ? (uint32_t)N : 1u) : kGroupMax; }

}  // namespace sweep

// class_sweep.hip: all pointers are device pointers.  ops uint32[n_ops][4]; reps uint32[S][ncls][W]; z double[S][ncls]: overwritten.
struct SweepArgs {
    uint32_t S;
    int ncls, W, width, n_ops;
    double wxz[4], scale;
};
hipError_t launch_class_sweep(const SweepArgs &a, const uint32_t *ops, const uint32_t *reps, double *z, hipStream_t stream);

}  // namespace qecmc
