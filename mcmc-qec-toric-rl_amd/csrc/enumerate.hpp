// The exact class law by coset enumeration.  Every chain with the syndrome of a given chain m is m times a logical operator times a stabilizer, so the
// weight of class c is a sum over the 2^rank elements of the stabilizer group.  Every weight this library knows depends on a chain only through
// n_xy = #X + #Y and n_z = #Z, so a class is summarised exactly by the integer histogram
//     H[c][n_xy][n_z] = number of chains of class c (the convention of qecmc_eq_class) with the syndrome that have those counts,
// uint64[ncls][nq+1][nq+1], every class summing to 2^rank.
//
// build_table(code, L) packs the code's generator table into X / Z bit planes, one bit per qubit of the nq-byte state layout (X bit: Paulis 1 and 2,
// Z bit: Paulis 2 and 3; the planar code's unused cells stay 0), keeps the generators greedy GF(2) elimination in table order finds independent -- THE
// BASIS: toric L = 3 16 of 18, planar all 2L(L-1), xzzx / rotated all L^2 - 1 -- and takes the logical operators and the class-move table from
// correct::build_table() (position 0): the representative of class c is the input times the kinds need[class of the input][c] names.
//
// ELEMENT ORDER (specified): element e in [0, 2^rank) is the product of the basis generators whose bit is set in e; chunk k of width chunk_bits is
// e in [k << chunk_bits, (k + 1) << chunk_bits).  A call enumerates chunks [chunk_first, chunk_first + chunk_count): partial histograms over disjoint
// ranges add up to the whole.  The order inside a chunk is the kernel's own business.
//
// Refused, before a device is looked for: QECMC_ERR_INVALID for a (code, L) check_code_L() does not know (xzzx / rotated at even L among them: their
// generator tables are defined for odd L only); QECMC_ERR_UNSUPPORTED for nq > kMaxQubits (the planes are one 32-bit word: no (code, L) the library
// knows has more than 32 qubits and a rank within kMaxRank), a rank above kMaxRank or below kMinChunkBits (planar L = 2), a (code, L) without a class
// move (the toric code at even L) and a histogram that does not fit lds_carve().  What is left today: toric L = 3; planar L = 3, 4; xzzx / rotated
// L = 3, 5.
//
// enumerate_host() is the twin of the kernel in enumerate.hip: a plain loop in element order.  The output is integer counts, so GPU = twin means equality.
#pragma once
#include "../../include/qecmc.h"

#include <cstdint>
#include <vector>

#include "corrections.hpp"     // the class function on the packed state, the logical masks and the class-move table
#include "plan_host.hpp"       // Refusal, check_code_L

namespace qecmc {
namespace enumr {

constexpr int kMaxQubits = 32, kMaxRank = 36;
constexpr int kMinChunkBits = 8, kMaxChunkBits = 30, kDefaultChunkBits = 24;
// the launch: kThreads per workgroup, at most kPairBudget (syndrome x element) pairs -- or one chunk of one syndrome where that is more -- and at most
// kGroupMax syndromes (the device histogram of a group is kGroupMax * ncls * (nq+1)^2 * 8 bytes at most, whatever N)
constexpr int kThreads = 256;
constexpr uint64_t kPairBudget = 1ull << 28;
constexpr uint32_t kGroupMax = 1024;
constexpr uint32_t kLdsBudget = 64 * 1024;   // the default dynamic-LDS window: two workgroups and more fit the 160 KiB of a CU

// The LDS of one workgroup: `copies` histograms of ncls * bins 32-bit counters, lane l adding into copy l % copies -- as many as fit the budget, up to
// four, to thin the same-address adds of one wave instruction; copies == 0: not even one fits.
struct Carve {
    uint32_t bins = 0, copy_words = 0, copies = 0, bytes = 0;
};
inline Carve lds_carve(int nq, int ncls)
{
    Carve c;
    c.bins = (uint32_t)(nq + 1) * (uint32_t)(nq + 1);
    c.copy_words = c.bins * (uint32_t)ncls;
    const uint32_t fit = kLdsBudget / (c.copy_words * 4u);
    c.copies = fit < 4u ? fit : 4u;
    c.bytes = c.copies * c.copy_words * 4u;
    return c;
}

struct Table {
    int code = 0, L = 0, nq = 0, W = 0, ncls = 0, kinds = 0, rank = 0;
    std::vector<uint32_t> gx, gz;      // [rank]: the basis generators' planes
    std::vector<uint32_t> kx, kz;      // [kinds]: the logical operators at position 0
    std::vector<uint32_t> need;        // [ncls][ncls]: correct::Table::need
    Carve carve;
    Refusal refusal;                   // code != 0: the (code, L) is refused, nothing else is filled in
};

inline Table build_table(int code, int L)
{
    Table t;
    t.code = code; t.L = L;
    if ((t.refusal = check_code_L(code, L)).code) return t;
    t.nq = code_nq_of(code, L);
    if (t.nq > kMaxQubits) {
        t.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "coset enumeration packs a chain into %d-bit planes: code %d at L=%d has %d qubits", kMaxQubits, code, L, t.nq);
        return t;
    }
    const correct::Table ct = correct::build_table(code, L);
    t.W = ct.W; t.ncls = ct.ncls; t.kinds = ct.kinds;
    // ---- the basis: greedy elimination over the 2 nq-bit vectors (x | z << 32), in table order
    std::vector<uint64_t> reduced, pivot;
    for (int g = 0; g < ct.n_gen; ++g) {
        uint32_t x = 0, z = 0;
        for (int i = 0; i < 4; ++i) {
            const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
            if (pauli == 0u) continue;
            if ((int)site >= t.nq) { t.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: generator %d of code %d at L=%d leaves the state", g, code, L); return t; }
            if (pauli == 1u || pauli == 2u) x ^= 1u << site;
            if (pauli >= 2u) z ^= 1u << site;
        }
        uint64_t v = (uint64_t)x | ((uint64_t)z << 32);
        for (size_t i = 0; i < reduced.size(); ++i)
            if (v & pivot[i]) v ^= reduced[i];
        if (v == 0) continue;                                                   // a product of earlier generators
        reduced.push_back(v); pivot.push_back(v & (~v + 1));                    // (its lowest set bit: no later vector keeps it)
        for (size_t i = 0; i + 1 < reduced.size(); ++i)
            if (reduced[i] & pivot.back()) reduced[i] ^= v;
        t.gx.push_back(x); t.gz.push_back(z);
    }
    t.rank = (int)t.gx.size();
    if (t.rank < kMinChunkBits) {
        t.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "the stabilizer group of code %d at L=%d has 2^%d elements: fewer than the smallest chunk, 2^%d", code, L, t.rank, kMinChunkBits);
        return t;
    }
    if (t.rank > kMaxRank) {
        t.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "the stabilizer group of code %d at L=%d has 2^%d elements: coset enumeration stops at 2^%d", code, L, t.rank, kMaxRank);
        return t;
    }
    if (ct.need.empty()) {
        t.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "no class move for code %d at L=%d: its logical operators do not reach every equivalence class (the toric code's "
                                                         "parity class does not see a logical line of even length)", code, L);
        return t;
    }
    t.carve = lds_carve(t.nq, t.ncls);
    if (t.carve.copies == 0) {
        t.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "the histogram of code %d at L=%d (%u counters) does not fit %u bytes of LDS", code, L, t.carve.copy_words, kLdsBudget);
        return t;
    }
    // ---- the logical operators at position 0, field by field of the 2-bit packed masks
    for (int kind = 0; kind < t.kinds; ++kind) {
        uint32_t x = 0, z = 0;
        for (int q = 0; q < t.nq; ++q) {
            const uint32_t f = (ct.masks[((size_t)kind * (L + 1)) * t.W + (q >> 4)] >> ((q & 15) * 2)) & 3u;
            if (f == 1u || f == 2u) x |= 1u << q;
            if (f >= 2u) z |= 1u << q;
        }
        t.kx.push_back(x); t.kz.push_back(z);
    }
    t.need = ct.need;
    return t;
}

// chunk_bits (0: the default; beyond the rank: the rank -- one chunk) and the range [chunk_first, chunk_first + chunk_count) (chunk_count 0: all from
// chunk_first) of a table build_table() accepted: resolved in place, or QECMC_ERR_INVALID
inline Refusal resolve_range(const Table &t, int &chunk_bits, uint64_t chunk_first, uint64_t &chunk_count)
{
    if (chunk_bits != 0 && (chunk_bits < kMinChunkBits || chunk_bits > kMaxChunkBits))
        return refuse_params(QECMC_ERR_INVALID, "chunk_bits=%d: 0 (the default) or %d .. %d", chunk_bits, kMinChunkBits, kMaxChunkBits);
    if (chunk_bits == 0) chunk_bits = kDefaultChunkBits;
    if (chunk_bits > t.rank) chunk_bits = t.rank;
    const uint64_t n_chunks = 1ull << (t.rank - chunk_bits);
    if (chunk_first >= n_chunks || chunk_count > n_chunks - chunk_first)
        return refuse_params(QECMC_ERR_INVALID, "chunks [%llu, +%llu) lie beyond the %llu chunks of 2^%d elements", (unsigned long long)chunk_first,
                             (unsigned long long)chunk_count, (unsigned long long)n_chunks, chunk_bits);
    if (chunk_count == 0) chunk_count = n_chunks - chunk_first;
    return {};
}

// the planes of the product of the basis generators [first_bit, rank) whose bit is set in `bits` (bit 0 of `bits`: generator first_bit)
inline void product_planes(const Table &t, int first_bit, uint64_t bits, uint32_t &x, uint32_t &z)
{
    x = z = 0;
    for (int b = first_bit; b < t.rank; ++b)
        if ((bits >> (b - first_bit)) & 1u) { x ^= t.gx[(size_t)b]; z ^= t.gz[(size_t)b]; }
}

// one chain uint8[nq]: its class, and the planes of the representative of every class -- reps uint32[ncls][2] (x, z)
inline int class_representatives(const Table &t, const uint8_t *chain, uint32_t *reps)
{
    uint32_t words[(kMaxQubits + 15) / 16] = {}, x = 0, z = 0;
    for (int q = 0; q < t.nq; ++q) {
        const uint32_t f = chain[q] & 3u;
        words[q >> 4] |= f << ((q & 15) * 2);
        if (f == 1u || f == 2u) x |= 1u << q;
        if (f >= 2u) z |= 1u << q;
    }
    lift::HostState st{words};
    const int a = correct::class_of(st, t.code, t.L, t.W);
    for (int c = 0; c < t.ncls; ++c) {
        uint32_t rx = x, rz = z;
        for (int kind = 0; kind < t.kinds; ++kind)
            if ((t.need[(size_t)a * t.ncls + c] >> kind) & 1u) { rx ^= t.kx[(size_t)kind]; rz ^= t.kz[(size_t)kind]; }
        reps[2 * c] = rx; reps[2 * c + 1] = rz;
    }
    return a;
}

inline int popcount32(uint32_t v) { return __builtin_popcount(v); }

// The twin.  chains uint8[N][nq] -> hist uint64[N][ncls][nq+1][nq+1] (overwritten) of the chunks [chunk_first, chunk_first + chunk_count) of width
// chunk_bits, as resolve_range() left them; cls int32[N] (nullable): the class of every input.  Element after element in element order: from e to
// e + 1 the generators of the bits that change.
inline void enumerate_host(const Table &t, uint64_t N, const uint8_t *chains, int chunk_bits, uint64_t chunk_first, uint64_t chunk_count, uint64_t *hist,
                           int32_t *cls)
{
    const size_t nq1 = (size_t)t.nq + 1, per = (size_t)t.ncls * nq1 * nq1;
    const uint64_t e0 = chunk_first << chunk_bits, n = chunk_count << chunk_bits;
    std::vector<uint32_t> reps((size_t)t.ncls * 2);
    for (uint64_t s = 0; s < N; ++s) {
        uint64_t *h = hist + s * per;
        for (size_t i = 0; i < per; ++i) h[i] = 0;
        const int a = class_representatives(t, chains + s * (uint64_t)t.nq, reps.data());
        if (cls) cls[s] = a;
        uint32_t x, z;
        product_planes(t, 0, e0, x, z);
        for (uint64_t i = 0; i < n; ++i) {
            for (int c = 0; c < t.ncls; ++c) {
                const uint32_t xx = x ^ reps[(size_t)2 * c], zz = z ^ reps[(size_t)2 * c + 1];
                ++h[((size_t)c * nq1 + (size_t)popcount32(xx)) * nq1 + (size_t)popcount32(zz & ~xx)];
            }
            const uint64_t flip = (e0 + i) ^ (e0 + i + 1);                      // (the last step runs into bit `rank` or beyond: no generator there)
            for (int b = 0; b < t.rank && ((flip >> b) & 1u); ++b) { x ^= t.gx[(size_t)b]; z ^= t.gz[(size_t)b]; }
        }
    }
}

// How one (group of syndromes, chunk) becomes a launch: S syndromes per group, 2^slice_bits elements per workgroup -- so many that a group's launch has
// about 2^10 workgroups where the chunk allows it, never fewer than one pass of the workgroup's threads.  T: the elements a thread walks, 2^T.
constexpr int walk_bits(int ncls) { return ncls == 16 ? 4 : 6; }
struct Shape {
    uint32_t group = 1, blocks = 1;
    int slice_bits = 0;
};
inline Shape launch_shape(int ncls, int chunk_bits, uint64_t N)
{
    Shape s;
    uint64_t g = kPairBudget >> chunk_bits;
    if (g < 1) g = 1;
    if (g > kGroupMax) g = kGroupMax;
    if (g > N) g = N ? N : 1;
    s.group = (uint32_t)g;
    int lg = 0;
    while ((2ull << lg) <= g) ++lg;                                             // floor(log2(group))
    const int pass_bits = walk_bits(ncls) + 8;                                  // one pass of kThreads = 2^8 threads
    const int most = chunk_bits > pass_bits ? chunk_bits : pass_bits;
    s.slice_bits = chunk_bits + lg - 10;
    if (s.slice_bits < pass_bits) s.slice_bits = pass_bits;
    if (s.slice_bits > most) s.slice_bits = most;
    s.blocks = chunk_bits > s.slice_bits ? 1u << (chunk_bits - s.slice_bits) : 1u;
    return s;
}

}  // namespace enumr

// enumerate.hip: all pointers are device pointers.  gen uint32[chunk_bits][2]: the planes (x, z) of the basis generators below the chunk; reps
// uint32[S][ncls][2]; hist uint64[S][ncls][bins]: ADDED to.  cx / cz: the product of the basis generators the chunk's index names.
struct EnumArgs {
    uint32_t S, nq1, bins, copies, cx, cz;
    int ncls, chunk_bits, slice_bits;
    uint32_t blocks;
};
hipError_t launch_enumerate(const EnumArgs &a, const uint32_t *gen, const uint32_t *reps, unsigned long long *hist, hipStream_t stream);

}  // namespace qecmc
