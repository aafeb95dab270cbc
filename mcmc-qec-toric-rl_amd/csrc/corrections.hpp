// From decoded syndromes to corrections: given K >= 1 candidate chains of one syndrome (all with that syndrome: not checked) and a target class t in
// the convention of qecmc_eq_class (the column order of counts / distr), correct_body() returns a chain with the same syndrome IN class t:
//   survey   class c_k and error count w_k of every candidate;
//   pick     some c_k == t: source = the lowest k of minimal w_k among those, moved = 0; else source = the lowest k of minimal w_k among all, moved = 1;
//   move     (moved only) multiply by the logical operators need[c_source][t] names -- a bit mask over the code's logical kinds, the kinds of the
//            [4][L+1][W] mask tables tables::toric_logical_masks / surf_logical_masks (4 on the torus, 2 elsewhere) -- in ascending kind; kind at position 0
//            (place == 0) or at the position p in [0, L) for which chain XOR mask[kind][p] has the lowest error count, ties to the lowest p (place != 0);
//   descend  (descend != 0) the lift's greedy descent (syndrome_lift.hpp greedy_descent): a local minimum of the weight within the class.
// status 0: corrected; 1: t outside [0, ncls) -- the chain is all zero, weight -1, source -1, moved 0.
//
// The class-move table need[ncls][ncls] is DERIVED on the host, not written down: every product of kinds at position 0 is applied to the zero chain and
// the class function read (the representative of that class); need[a][b] is the product that takes the representative of a to class b.  If the 2^kinds
// products do not reach ncls distinct classes the table is empty and the entry points refuse the (code, L) with QECMC_ERR_UNSUPPORTED.  Among the
// (code, L) check_code_L() accepts (L in [2, 64]; xzzx / rotated: odd L) that is exactly THE TORIC CODE AT EVEN L: the reference's class is the parity
// of the X / Z components over a layer, and a logical line of even length does not change it (cf. cdelta = (L & 1) ? ... : 0 in the colour body).  The
// toric code at odd L, the xzzx and rotated codes at every odd L and the planar code at every L are supported (checked by build_table() over the
// whole range: corrections_selftest.cpp).
//
// The table builder is pure host C++.  correct_body() is ONE __host__ __device__ function: corrections.hip runs it with one lane per syndrome and the
// state in LDS, tables_test_api.cpp and corrections_selftest.cpp run it by g++ on a plain array -- the tests compare the two bit for bit.
#pragma once
#include "../../include/qecmc.h"

#include <cstdint>
#include <vector>

#include "stencil_bytes.hpp"   // code_nq_of: the codes' dimensions
#include "syndrome_lift.hpp"   // count_fields, greedy_descent, HostState
#include "tables.hpp"          // the logical masks and the generator tables

namespace qecmc {
namespace correct {

__host__ __device__ inline uint32_t parity32(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v) & 1u;
#else
    return (uint32_t)__builtin_popcount(v) & 1u;
#endif
}

// The class functions of stencil_bytes.hpp (toric_eq_class_b / surf_eq_class_b) on the packed state, as ladder_colour_body.inc states them: toric -- the
// parities of the X and Z components over each layer; the others -- the X / Z components along the first row and the first column (xzzx: alternating,
// and the class is v ^ (v >> 1) of v = x | z << 1).  Every word index depends on the loop counters only.
template <class St>
__host__ __device__ inline int class_of(const St &st, int code, int L, int W)
{
    if (code == kCodeToric) {
        const int LL = L * L, wb = LL >> 4;
        const uint32_t lowmask = (1u << ((LL & 15) * 2)) - 1u;
        uint32_t acc0 = 0, acc1 = 0;
        for (int w = 0; w < W; ++w) {
            const uint32_t x = st.get(w);
            if (w < wb) acc0 ^= x;
            else if (w > wb) acc1 ^= x;
            else { acc0 ^= x & lowmask; acc1 ^= x & ~lowmask; }
        }
        return (int)(parity32((acc0 ^ (acc0 >> 1)) & 0x55555555u) + 2u * parity32(acc0 & 0xAAAAAAAAu) + 4u * parity32((acc1 ^ (acc1 >> 1)) & 0x55555555u) +
                     8u * parity32(acc1 & 0xAAAAAAAAu));
    }
    uint32_t x = 0, z = 0;
    for (int i = 0; i < L; ++i) {
        const uint32_t qa = (uint32_t)i, qb = (uint32_t)(i * L);
        const uint32_t fa = (st.get((int)(qa >> 4)) >> ((qa & 15u) * 2u)) & 3u, fb = (st.get((int)(qb >> 4)) >> ((qb & 15u) * 2u)) & 3u;
        const uint32_t xa = (fa ^ (fa >> 1)) & 1u, za = fa >> 1, xb = (fb ^ (fb >> 1)) & 1u, zb = fb >> 1;
        if (code == kCodeXzzx) { x ^= (i & 1) ? za : xa; z ^= (i & 1) ? xb : zb; }
        else if (code == kCodePlanar) { x ^= xb; z ^= za; }
        else { x ^= xa; z ^= zb; }
    }
    const uint32_t v = x | (z << 1);
    return (int)(code == kCodeXzzx ? v ^ (v >> 1) : v);
}

// The tables of one (code, L).  masks: [4][L+1][W] as tables::*_logical_masks build them (kinds >= `kinds` unused, position L the identity);
// need: [ncls][ncls] bit masks over the kinds; gen: the generator table, 2 words each.  need empty: the (code, L) has no class move (header comment).
struct Table {
    int code = 0, L = 0, nq = 0, W = 0, ncls = 0, kinds = 0, n_gen = 0;
    std::vector<uint32_t> masks, need, gen;
};

inline Table build_table(int code, int L)
{
    Table t;
    t.code = code; t.L = L; t.nq = code_nq_of(code, L); t.W = (t.nq + 15) / 16;
    t.ncls = code == QECMC_TORIC ? 16 : 4;
    t.kinds = code == QECMC_TORIC ? 4 : 2;
    t.masks = code == QECMC_TORIC ? tables::toric_logical_masks(L, t.W) : tables::surf_logical_masks(code, L, t.W);
    t.gen = code == QECMC_TORIC ? tables::toric_generator_table(L) : tables::surf_generator_table(code, L);
    t.n_gen = (int)(t.gen.size() / 2);
    const int n_prod = 1 << t.kinds;
    std::vector<uint32_t> words((size_t)t.W);
    lift::HostState st{words.data()};
    // the class of product m applied to the chain `from` -- itself a product applied to the zero chain (0: the zero chain); a mask applied twice cancels
    auto class_after = [&](int from, int m) {
        for (int w = 0; w < t.W; ++w) words[(size_t)w] = 0u;
        for (int kind = 0; kind < t.kinds; ++kind)
            if (((from >> kind) ^ (m >> kind)) & 1)
                for (int w = 0; w < t.W; ++w) words[(size_t)w] ^= t.masks[((size_t)kind * (L + 1)) * t.W + w];
        return class_of(st, code, L, t.W);
    };
    if (class_after(0, 0) != 0) return t;                                   // (the zero chain is in class 0 in every model)
    std::vector<int> rep((size_t)t.ncls, -1);                               // class -> the product that reaches it from the zero chain
    for (int m = 0; m < n_prod; ++m) {
        const int c = class_after(0, m);
        if (c < 0 || c >= t.ncls) return t;
        if (rep[(size_t)c] < 0) rep[(size_t)c] = m;
    }
    for (int c = 0; c < t.ncls; ++c)
        if (rep[(size_t)c] < 0) return t;                                   // fewer than ncls classes reached: no class move
    std::vector<uint32_t> need((size_t)t.ncls * t.ncls, 0u);
    for (int a = 0; a < t.ncls; ++a)
        for (int b = 0; b < t.ncls; ++b) {
            int found = -1;
            for (int m = 0; m < n_prod && found < 0; ++m)
                if (class_after(rep[(size_t)a], m) == b) found = m;         // product m on the representative of a
            if (found < 0) return t;
            need[(size_t)a * t.ncls + b] = (uint32_t)found;
        }
    t.need = need;
    return t;
}

// One syndrome.  St as in lift_body(): get(w), set(w, v), any(b).  cand: this syndrome's K candidates uint8[K][nq], or nullptr for an idle lane (its
// state stays zero, its outputs are not to be used).  The K candidates pass through the ONE state st holds: each is packed into it, surveyed and
// overwritten by the next; the chosen one is packed again.  Every table address depends on kernel arguments and loop counters only -- a lane's own
// class, target, kinds and position only predicate what it does.
template <class St>
__host__ __device__ inline void correct_body(St &st, const uint32_t *__restrict__ masks, const uint32_t *__restrict__ need, const uint32_t *__restrict__ gen,
                                             int code, int L, int W, int nq, int n_gen, int ncls, int kinds, const uint8_t *__restrict__ cand, int K, int target,
                                             int place, int descend, int &weight, int &source, int &moved, int &status)
{
    auto load = [&](int k) {
        for (int w = 0; w < W; ++w) {
            uint32_t word = 0;
            if (cand != nullptr)
                for (int b = 0; b < 16; ++b) {
                    const int q = w * 16 + b;
                    if (q < nq) word |= (uint32_t)(cand[(size_t)k * (size_t)nq + (size_t)q] & 3u) << (2 * b);
                }
            st.set(w, word);
        }
    };
    auto count = [&]() {
        int n = 0;
        for (int w = 0; w < W; ++w) n += lift::count_fields(st.get(w));
        return n;
    };
    status = (target < 0 || target >= ncls) ? 1 : 0;
    const bool active = cand != nullptr && status == 0;
    // ---- survey and pick
    int in_k = -1, in_w = 0, all_k = 0, all_w = 0, all_c = 0;
    for (int k = 0; k < K; ++k) {
        load(k);
        const int c = class_of(st, code, L, W), n = count();
        if (k == 0 || n < all_w) { all_k = k; all_w = n; all_c = c; }
        if (c == target && (in_k < 0 || n < in_w)) { in_k = k; in_w = n; }
    }
    moved = active && in_k < 0 ? 1 : 0;
    source = !active ? -1 : in_k >= 0 ? in_k : all_k;
    if (K > 1) load(source < 0 ? 0 : source);
    if (!active)
        for (int w = 0; w < W; ++w) st.set(w, 0u);
    // ---- move: the kinds need[class of the source][target] names
    uint32_t todo = 0;
    for (int a = 0; a < ncls; ++a)
        for (int b = 0; b < ncls; ++b) {
            const uint32_t v = need[a * ncls + b];
            if (moved && a == all_c && b == target) todo = v;
        }
    const int n_pos = place ? L : 1;
    for (int kind = 0; kind < kinds; ++kind) {
        const bool mine = ((todo >> kind) & 1u) != 0u;
        if (!st.any(mine)) continue;
        const uint32_t *row = masks + (size_t)kind * (size_t)(L + 1) * (size_t)W;
        int best_p = 0, best_n = 0;
        for (int p = 0; p < n_pos; ++p) {
            int n = 0;
            for (int w = 0; w < W; ++w) n += lift::count_fields(st.get(w) ^ row[(size_t)p * (size_t)W + w]);
            if (p == 0 || n < best_n) { best_p = p; best_n = n; }
        }
        for (int p = 0; p < n_pos; ++p)
            for (int w = 0; w < W; ++w) {
                const uint32_t m = row[(size_t)p * (size_t)W + w];
                if (m == 0u) continue;                                   // (the same for every syndrome: most words of a line are empty)
                if (mine && p == best_p) st.set(w, st.get(w) ^ m);
            }
    }
    if (descend) lift::greedy_descent(st, gen, nq, n_gen);
    weight = status ? -1 : count();
}

// N syndromes on the host, one after the other: candidates uint8[N][K][nq], target int32[N] -> corrections uint8[N][nq], weight / source int32[N],
// moved / status uint8[N] (the last four nullable)
inline void corrections_host(const Table &t, uint64_t N, uint32_t K, const uint8_t *candidates, const int32_t *target, int place, int descend,
                             uint8_t *corrections, int32_t *weight, int32_t *source, uint8_t *moved, uint8_t *status)
{
    std::vector<uint32_t> words((size_t)t.W);
    lift::HostState st{words.data()};
    for (uint64_t s = 0; s < N; ++s) {
        int wgt = 0, src = 0, mov = 0, stat = 0;
        correct_body(st, t.masks.data(), t.need.data(), t.gen.data(), t.code, t.L, t.W, t.nq, t.n_gen, t.ncls, t.kinds,
                     candidates + s * (uint64_t)K * (uint64_t)t.nq, (int)K, target[s], place, descend, wgt, src, mov, stat);
        for (int q = 0; q < t.nq; ++q) corrections[s * (uint64_t)t.nq + q] = (uint8_t)((words[(size_t)(q >> 4)] >> ((q & 15) * 2)) & 3u);
        if (weight) weight[s] = wgt;
        if (source) source[s] = src;
        if (moved) moved[s] = (uint8_t)mov;
        if (status) status[s] = (uint8_t)stat;
    }
}

}  // namespace correct

// corrections.hip: all pointers are device pointers; weight / source / moved / status nullable.  One lane per syndrome, 64-lane workgroups,
// W * 256 bytes of LDS: one resident state per lane.
struct CorrectArgs {
    uint64_t N;
    int code, L, W, nq, n_gen, ncls, kinds, K, place, descend;
};
hipError_t launch_corrections(const CorrectArgs &a, const uint32_t *masks, const uint32_t *need, const uint32_t *gen, const uint8_t *candidates,
                              const int32_t *target, uint8_t *corrections, int32_t *weight, int32_t *source, uint8_t *moved, uint8_t *status,
                              hipStream_t stream);

}  // namespace qecmc
