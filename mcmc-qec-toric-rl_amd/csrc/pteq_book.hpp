// The reference's PTEQ bookkeeping and its error_based stopping rule (decoders.py:60-82,93-105; decoders_biasednoise.py:204,229-238), and
// how one ladder's results reach its syndrome's row, for ladder_kernel.hpp, ladder_colour.hpp and ladder_wu.hpp.  Plain device functions on
// values: where a kernel keeps its counters is the caller's business.  Where a call changed a kernel's resource row the rule stays in place, marked there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qecmc {

// slot record published once per ladder step: error count | state id << 16 | class << 24 | flag << 31
// (flag = "has been at the top since it last reached the bottom", Chain.flag, mcmc.py:75,99-103)
__device__ __forceinline__ uint32_t pack_info(uint32_t n, uint32_t sid, uint32_t cls, uint32_t flag)
{
    return n | (sid << 16) | (cls << 24) | (flag << 31);
}
__device__ __forceinline__ uint32_t info_n(uint32_t r) { return r & 0xFFFFu; }
__device__ __forceinline__ uint32_t info_sid(uint32_t r) { return (r >> 16) & 0xFFu; }
__device__ __forceinline__ uint32_t info_cls(uint32_t r) { return (r >> 24) & 0x3Fu; }
__device__ __forceinline__ uint32_t info_flag(uint32_t r) { return r >> 31; }

// The series nbr_errors_bottom_chain[since_burn] (decoders.py:68; alpha noise: chains[0].n_eff, decoders_biasednoise.py:204, logged as
// n_z | (n_x + n_y) << 16) is logged in HBM, series index i in row burn + i, and the criterion compares the means of its quartile
// windows Q2 = series[l/4 : l/2] and Q4 = series[3l/4 : l] (:93-105).  Their sums are carried: when the series grows to l samples the
// new value enters Q4, row c0 leaves it if c1 != c0, row b0 enters Q2 if b1 != b0 and row a0 leaves Q2 if a1 != a0.
struct QuartileRows { uint32_t a0, b0, c0, a1, b1, c1; };
__device__ __forceinline__ QuartileRows quartile_rows(uint32_t l)
{
    const uint32_t lo1 = l - 1;
    return {lo1 >> 2, lo1 >> 1, (3u * lo1) >> 2, l >> 2, l >> 1, (3u * l) >> 2};
}
// v0: the value logged now; vc, vb, va: the log's rows c0, b0, a0 -- 0 for a row that does not move.  sumA / sumB: the sums of Q2 / Q4
// (alpha noise: of n_z, and sumAxy / sumBxy of n_x + n_y): exact integers.
template <bool ALPHA>
__device__ __forceinline__ void window_update(uint32_t v0, uint32_t vc, uint32_t vb, uint32_t va, uint64_t &sumA, uint64_t &sumB,
                                              uint64_t &sumAxy, uint64_t &sumBxy)
{
    if constexpr (ALPHA) {
        sumB += v0 & 0xFFFFu; sumBxy += v0 >> 16;
        sumB -= vc & 0xFFFFu; sumBxy -= vc >> 16;
        sumA += vb & 0xFFFFu; sumAxy += vb >> 16;
        sumA -= va & 0xFFFFu; sumAxy -= va >> 16;
    } else {
        sumB += v0; sumB -= vc; sumA += vb; sumA -= va;
    }
}

// n_eff = n_z + alpha (n_x + n_y) of a record n_z | n_xy << 16 as Chain_alpha forms it (mcmc_alpha.py:22,58; alpha_flip rebuilds it the same way): the one
// spelling every layout uses (product and sum rounded separately, as the reference's and the oracle's double arithmetic does)
__device__ __forceinline__ double alpha_neff(uint32_t rec, double alpha)
{
#pragma clang fp contract(off)
    return (double)(rec & 0xFFFFu) + alpha * (double)(rec >> 16);
}

// conv_crit_error_based_PT_alpha, decoders_biasednoise.py:229-238: |mean Q2 - mean Q4| < eps on the n_eff series, each mean
// formed as (sum n_z + alpha sum n_xy) / len from exact integer sums
__device__ inline bool alpha_series_close(uint64_t z2, uint64_t xy2, uint32_t den2, uint64_t z4, uint64_t xy4, uint32_t den4,
                                          double alpha, double eps)
{
#pragma clang fp contract(off)
    const double q2 = ((double)z2 + alpha * (double)xy2) / (double)den2;
    const double q4 = ((double)z4 + alpha * (double)xy4) / (double)den4;
    return fabs(q2 - q4) < eps;
}

// conv_crit_error_based_PT (decoders.py:93-105) on `samples` logged values: |mean Q2 - mean Q4| < eps; an empty slice -> nan -> not accepted
template <bool ALPHA>
__device__ __forceinline__ bool criterion_accepts(uint32_t samples, uint64_t sumA, uint64_t sumAxy, uint64_t sumB, uint64_t sumBxy,
                                                  double alpha, double eps)
{
    const uint32_t l = samples ? samples : 1u;
    const uint32_t den2 = (l >> 1) - (l >> 2), den4 = l - ((3u * l) >> 2);
    if (!(samples && den2 && den4)) return false;
    if constexpr (ALPHA) return alpha_series_close(sumA, sumAxy, den2, sumB, sumBxy, den4, alpha, eps);
    else return fabs((double)sumA / (double)den2 - (double)sumB / (double)den4) < eps;   // :96-102
}

// decoders.py:74-82, once tops0 >= TOPS: the criterion has to hold while tops0 advances by SEQ.  True: the ladder has converged (:77-78)
__device__ __forceinline__ bool streak_ends(bool accept, uint32_t tops0, uint32_t SEQ, uint32_t &conv_start, uint32_t &conv_streak)
{
    if (accept) {
        if (conv_streak >= SEQ) return true;
        conv_streak = tops0 - conv_start;                                               // :79
    } else {
        conv_streak = 0;                                                                // :81-82
        conv_start = tops0;
    }
    return false;
}

// One ladder's results into row `row` of its syndrome's outputs (any of them may be null).  replicas > 1: the syndrome's ladders are summed
// with atomics into rows the caller zeroed -- steps_done their maximum, converged (preset 1) cleared by a ladder that did not converge;
// else plain stores, samples added to what is there if `accumulate`.
__device__ __forceinline__ void store_ladder_results(uint32_t *samples_out, uint32_t *tops0_out, uint32_t *steps_done_out, uint8_t *converged_out,
                                                     uint64_t row, uint32_t replicas, bool accumulate, uint32_t samples, uint32_t tops0,
                                                     uint32_t steps_done, bool converged)
{
    if (replicas > 1) {
        if (samples_out != nullptr) atomicAdd(samples_out + row, samples);
        if (tops0_out != nullptr) atomicAdd(tops0_out + row, tops0);
        if (steps_done_out != nullptr) atomicMax(steps_done_out + row, steps_done);
        if (converged_out != nullptr && !converged) converged_out[row] = 0;
    } else {
        if (samples_out != nullptr) samples_out[row] = accumulate ? samples_out[row] + samples : samples;
        if (tops0_out != nullptr) tops0_out[row] = tops0;
        if (steps_done_out != nullptr) steps_done_out[row] = steps_done;
        if (converged_out != nullptr) converged_out[row] = (uint8_t)converged;
    }
}
// ... and classes c_first, c_first + c_step, ... of its histogram (class c at col[c * stride]) into its row of counts; `clear` zeroes them
__device__ __forceinline__ void store_class_column(uint32_t *counts_row, uint32_t *col, int stride, int c_first, int c_step, int ncls,
                                                   uint32_t replicas, bool clear)
{
    for (int c = c_first; c < ncls; c += c_step) {
        const uint32_t v = col[c * stride];
        if (clear) col[c * stride] = 0;
        if (replicas > 1) { if (v) atomicAdd(counts_row + c, v); }
        else counts_row[c] = v;
    }
}

// Issue arbitration between co-resident workgroups is oldest-first, which lets the first one
// race ahead and leaves the last one alone (latency-bound, 2 waves per SIMD) at the end of a
// launch.  Lowering a workgroup's priority as it advances (cyclically, every 8 steps) narrows
// that spread: +6 % on a one-round grid (measured), neutral otherwise.
// (Tried in round 2: the top-role wave at the highest priority instead: -10 % at L = 9, +3 % at L = 15, 0 at rotated L = 21.)
__device__ __forceinline__ void set_step_priority(uint64_t t)
{
    switch (3u - (uint32_t)((t >> 3) & 3)) {    // s_setprio takes an immediate
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}

}  // namespace qecmc
