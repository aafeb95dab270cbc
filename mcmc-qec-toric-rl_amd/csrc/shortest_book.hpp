// The shortest-chain statistics of PTEQ_alpha_with_shortest (decoders_biasednoise.py:93-172) for the kernels that book slot 0 themselves
// (ladder_wu.hpp SHORT, ladder_colour_body.inc SHORT).  After every ladder step past burn-in the reference looks at the bottom slot: c = the class of its
// configuration, v = its n_eff ATTRIBUTE (the slot's, possibly stale: Q4).  v < shortest[c]: a new minimum, shortest_n[c] = 1, unique[c] = {config}
// (:130-138); v == shortest[c]: shortest_n[c] += 1 and the configuration joins unique[c] (:139-144).  The minimum only falls, so the final unique[c] is the
// set of distinct configurations among the samples whose attribute equals the FINAL minimum: no set is ever emptied here -- a counter restarts at a new
// minimum, and one set per ladder tells fresh from seen.  Its key is a 64-bit mix of the configuration's packed words AND the bits of the double v (the
// same configuration may come with attributes of different value; with equal values the reference's dict holds it once); 0 means "empty".
// Plain device functions on values and on the caller's pointers: where a kernel keeps the kShortRows words of a ladder is its own business.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace qecmc {

// a ladder's state word of row `row` before its first sample: minima at the reference's sentinel 100000 (:113), everything else 0
__device__ __forceinline__ uint32_t short_init_word(int row) { return row < 16 && (row & 3) == 1 ? 0x40F86A00u : 0u; }   // (100000.0 = 0x40F86A00'00000000)

// the finaliser of splitmix64: every input bit reaches every output bit
__device__ __forceinline__ uint64_t short_mix(uint64_t h)
{
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    return h ^ (h >> 31);
}
// a sequential key (one lane holds the words): absorb word after word ...
constexpr uint64_t kShortKeySeed = 0xCBF29CE484222325ull;
__device__ __forceinline__ uint64_t short_key_word(uint64_t h, uint32_t word)
{
    h = (h ^ word) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
// ... a position-wise key (the lanes of a wave hold a word each): the XOR over the words of these
__device__ __forceinline__ uint64_t short_key_at(uint32_t pos, uint32_t word) { return short_mix(((uint64_t)(pos + 1u) << 32) | word); }
// ... and either with the value's 64 bits; never 0
__device__ __forceinline__ uint64_t short_key_finish(uint64_t h, double v)
{
    h = short_mix(h ^ short_mix((uint64_t)__double_as_longlong(v)));
    return h ? h : 1ull;
}

// Offer `key` to the ladder's own open-addressing table (`slots` words, a power of two >= 2 cap; one lane per table, so the CAS never competes).  True: the
// key was not there.  A ladder may offer `cap` distinct keys; the next fresh one sets `over` and is not stored, so the table never fills and a probe ends.
__device__ inline bool short_offer(unsigned long long *set, uint32_t slots, uint32_t cap, uint64_t key, uint32_t &offered, uint32_t &over)
{
    uint32_t i = (uint32_t)key & (slots - 1u);
    for (uint32_t probe = 0; probe < slots; ++probe) {
        unsigned long long prev;
        if (offered < cap) {
            prev = atomicCAS(set + i, 0ull, (unsigned long long)key);
            if (prev == 0ull) { offered += 1u; return true; }
        } else {
            prev = __hip_atomic_load(set + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev == 0ull) { over = 1u; return true; }
        }
        if (prev == (unsigned long long)key) return false;
        i = (i + 1u) & (slots - 1u);
    }
    over = 1u;
    return true;
}

// One post-burn sample of ladder `lad`: class c, attribute value v, key.  st: the ladder's row 0, rows `stride` words apart (kernel_choice.hpp kShortRows).
template <class P>
__device__ __forceinline__ void short_book(const LadderArgs &a, uint64_t lad, P st, int stride, uint32_t c, double v, uint64_t key)
{
    P sc = st + (4u * c) * (uint32_t)stride;
    const double mn = __hiloint2double((int)sc[stride], (int)sc[0]);
    if (!(v <= mn)) return;
    uint32_t offered = st[16 * stride], over = st[17 * stride];
    const bool fresh = short_offer(a.short_set + lad * (uint64_t)a.short_slots, a.short_slots, a.short_cap, key, offered, over);
    if (v < mn) {                                                                  // :130-138
        sc[0] = (uint32_t)__double2loint(v); sc[stride] = (uint32_t)__double2hiint(v);
        sc[2 * stride] = 1u; sc[3 * stride] = 1u;
    } else {                                                                       // :139-144
        sc[2 * stride] = sc[2 * stride] + 1u;
        if (fresh) sc[3 * stride] = sc[3 * stride] + 1u;
    }
    st[16 * stride] = offered; st[17 * stride] = over;
}

// the ladder's rows of qecmc_plan_set_shortest's outputs
template <class P>
__device__ __forceinline__ void short_store(const LadderArgs &a, uint64_t lad, P st, int stride)
{
    for (int c = 0; c < 4; ++c) {
        P sc = st + (4 * c) * stride;
        a.short_neff[lad * 4u + c] = __hiloint2double((int)sc[stride], (int)sc[0]);
        a.short_n[lad * 4u + c] = sc[2 * stride];
        a.short_uniq[lad * 4u + c] = sc[3 * stride];
    }
    a.short_over[lad] = (uint8_t)st[17 * stride];
}

}  // namespace qecmc
