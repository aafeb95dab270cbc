// scan = 3 (ladder_wu.hpp), the swap sweep's test as a BOUND.  Slots i and i + 1 trade states iff d <= 0 || x < ceil(p_diff[i]^d 2^32) with d = ne_hi - ne_lo
// (mcmc.py:146-149).  The thresholds fall with d and x -- a Philox word addressed by (T, block, ladder) -- depends on nothing the step computes, so the
// test reads d <= D_i(x) with D_i(x) the largest d in [0, nq] with d == 0 || x < swap_thr[i][d], and D_i(x) is found where x is drawn, off the cascade's
// serial path (ladder_kernel.hpp's swap_dmax is the same idea in the lane-per-chain kernel).  Host and device share the functions below
// (tests/test_wave_swap_bound_cpu.py runs them through tables_test_api.cpp against the brute-force maximum).
//
// The tables: near(d), 0 <= d < kSwapFast, is entry d of the pair's row of swapT as the kernels stage it (the thresholds of d = 1 .. min(nq, kSwapFast - 1);
// entry 0 and the entries past nq are 0), far(d), 1 <= d <= nq, the plan's swap_thr[i][d] -- 32 bits: swap_fast_ok.
#pragma once
#include <math.h>
#include <stdint.h>

#include "kernel_choice.hpp"

namespace qecmc {

// The guess and its check, without a branch.  x < ceil(p^d 2^32) iff d < log2(x / 2^32) / log2 p, so g = floor((log2(x + 1/2) - 32) inv) with
// inv = LadderArgs::swap_inv_log2[i] IS the bound unless the quotient lies within single precision's error of an integer (or x is so small that the
// thresholds are a few units apart, or have saturated at 1).  One window of two adjacent entries says which: D = g iff near(g + 1) <= x < near(g), one
// unsigned compare of two differences -- entry 0 is 0 and stands for 2^32 there, the differences wrap --, given that the row falls with d.  g is kept
// below kSwapFast - 1, so the window always lies in the row; a bound beyond it fails the check like any other miss.
// (in two halves, so that a drawer can have the reads of several words in flight at once: the guess, then the check on the two entries)
__host__ __device__ __forceinline__ uint32_t wu_swap_first(uint32_t x, float inv, int nq)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float l2 = __log2f((float)x + 0.5f);
#else
    const float l2 = log2f((float)x + 0.5f);
#endif
    const int hi = nq < kSwapFast - 2 ? nq : kSwapFast - 2;
    const float r = (l2 - 32.0f) * inv;
    return (uint32_t)(int)fminf(fmaxf(r, 0.0f), (float)hi);           // (fmaxf drops a NaN -- 0 inf, rungs that coincide: no plan of these kernels has them)
}
__host__ __device__ __forceinline__ bool wu_swap_holds(uint32_t x, uint32_t t0, uint32_t t1) { return x - t1 < t0 - t1; }   // t0 = near(g), t1 = near(g + 1)
// Returns the check, g the guess.
template <class Near>
__host__ __device__ __forceinline__ bool wu_swap_guess(uint32_t x, float inv, int nq, Near &&near, uint32_t &g)
{
    g = wu_swap_first(x, inv, nq);
    return wu_swap_holds(x, near((int)g), near((int)g + 1));
}

// From any start d in [0, nq] to D_i(x): up while the next entry passes, down while this one does not.  Exact for a row that falls with d.
template <class Near, class Far>
__host__ __device__ __forceinline__ uint32_t wu_swap_walk(uint32_t x, uint32_t start, int nq, Near &&near, Far &&far)
{
    auto below = [&](int dd) -> bool { return dd < kSwapFast ? x < near(dd) : x < far(dd); };
    int d = (int)start;
    while (d < nq && below(d + 1)) ++d;
    while (d > 0 && !below(d)) --d;
    return (uint32_t)d;
}

// D_i(x), exactly, whatever the guess
template <class Near, class Far>
__host__ __device__ __forceinline__ uint32_t wu_swap_bound(uint32_t x, float inv, int nq, Near &&near, Far &&far)
{
    uint32_t g;
    if (wu_swap_guess(x, inv, nq, near, g)) return g;
    return wu_swap_walk(x, g, nq, near, far);
}

// the sweep's rule on a bound: ne_hi - ne_lo <= D (the records' low 16 bits are the error counts, pack_info)
__host__ __device__ __forceinline__ bool wu_bound_flips(uint32_t car, uint32_t lo, uint32_t bound)
{
    return (int)(car & 0xFFFFu) - (int)(lo & 0xFFFFu) <= (int)bound;
}

}  // namespace qecmc
