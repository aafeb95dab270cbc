// scan = 2 (QECMC_SCAN_COLOUR): the latency layout.  One workgroup per LADDER (one syndrome), one wavefront per rung, the lanes
// of a wavefront = the stabilizer generators of one colour phase, proposed all at once.
//
// The reference decodes ONE syndrome per call (decoders.py:25, generate_data.py:136).  The throughput kernels (ladder_kernel.hpp)
// give every chain one lane and advance it one proposal at a time -- 64 syndromes per wavefront; a single syndrome then waits for
// 162 sequential proposals per sweep at L = 9.  Here the parallelism is inside the chain (BASELINE.json's north star:
// "thread-block per syndrome, checkerboard-parallel stabilizer flips, wavefront reductions for the dE count"): generators that
// share no qubit commute and their Metropolis tests are independent, so a whole phase of them is one wavefront instruction
// stream; a sweep is n_phases of those (7 at toric L = 9) instead of 162 proposals.
//
// This is NOT the reference's Markov chain (a systematic scan, like scan = 1): every single-generator Metropolis kernel keeps
// the rung's stationary law, hence so does their composition.  The rule, which the CPU oracle restates (scan = 2 of its model):
//   * the plan cuts the generators into phases (tables.hpp colour_phases: greedy colouring in table order, chunks of <= 64);
//     phase index K of a rung counts from prop0 = step0 * iters; a ladder step = `iters` phases of every rung, phase K uses
//     phase (K mod n_phases) of the table;
//   * top rung (slot Nc - 1, p_logical > 0; it sits at p = 0.75 where every move is accepted, mcmc.py:30): before the phase, with
//     probability p_logical (word 0 of block (K, 0) < ceil(p_logical 2^32)) one uniformly random logical operator drawn from
//     words 1-3 of that block exactly as scan = 1 draws it (toric_model.py:228-253 / xzzx_model.py:340-357);
//   * generator i of the phase draws u = word (K & 3) of block (K >> 2, 8 + i) of the rung's stream (the slot's own for the
//     top rule, the diagonal stream kDiagStream + (slot + step) mod Nc otherwise, as in the other scans);
//     a rung with f < 1 accepts iff u < ceil(f^dE 2^32) (dE <= 0: always; mcmc.py:42); a rung with f >= 1 (where a
//     coin-less sweep would compose to the identity) applies the generator iff the top bit of u is set;
//   * swap sweep, tops0 / class histogram bookkeeping: mcmc.py:94-103 and decoders.py:60-68 unchanged (swap uniforms: word i & 3
//     of block (t, i >> 2) of the swap stream, as in the other scans).
// conv_mode = error_based runs the reference's criterion on wave 0 (the workgroup leaves when its ladder has converged).  In
// fixed-length runs steps_done reports the first ladder step after which tops0 >= TOPS (or `steps`), converged whether it was
// reached: the "time to tops0 >= 10" the latency table of profiles/ quotes.
//
// RULE = 1 / 2: the biased (src/mcmc_biased.py) and alpha (src/mcmc_alpha.py) noise models on the xzzx / rotated codes.  The members of
// a phase are tested at once, so Q3's frozen p_b cannot be carried (a member's ratio would depend on what the members before it did):
// every generator is a Metropolis move for the model's own weight, u < (px / pI)^dxy (pz / pI)^dz with (dxy, dz) the change of
// n_x + n_y and n_z of that generator alone -- an 81-entry threshold table per rung (a.col_thr) --, the law the reference's rule has at
// iters = 1.  The biased top rung is not uniform: it runs the same rule and tests its logical operators (word 0 of block (K, 1) against
// the ratio of the power tables' products, the reference's expression); Ladder_alpha's top rung (pz_tilde = 1: every ratio is 1) takes
// the coin and its logical operators unseen, like the depolarizing one.  RULE = 2 also: the swap test on the slots' n_eff attributes
// (mcmc_alpha.py:118-123), which stay with the slot (Q4: a wave IS a slot here, the attribute is a scalar of the wave) and follow the
// counts only when a move was accepted (:58,:70); the criterion on the logged attribute of slot 0 (decoders_biasednoise.py:204,229-238).
#pragma once
#include "ladder_kernel.hpp"
#include "shortest_book.hpp"

namespace qecmc {

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// CONV: the error_based convergence criterion of decoders.py:74-82,93-105 on wave 0 (one ladder per workgroup: the workgroup leaves when
// its ladder has converged); steps_done / converged are then the criterion's, as in the other scans.
// Diagnostic build only (tools/steptrace.hip): shader-clock stamps of workgroup 0's waves at the phase boundaries of ladder steps 2000 .. 2031
#ifdef QECMC_STEPTRACE
#define QECMC_CSTAMP(k)                                                                                                        \
    do {                                                                                                                       \
        if (a.dbg && blockIdx.x == 0 && t >= 2000 && t < 2032 && lane == 0)                                                    \
            a.dbg[(size_t)gridDim.x * 4 + (((t - 2000) * 16 + slot) * 8 + (k))] = (k) == 5 ? (uint64_t)slot : (uint64_t)clock64(); \
    } while (0)
#else
#define QECMC_CSTAMP(k) ((void)0)
#endif

// MAXT / MINW: 1 024 threads at 4 waves per SIMD whatever the ladder's length (choose_colour, kernel_choice.hpp)
template <int CODE, bool CONV, int RULE = 0, int MAXT = 1024, int MINW = 4>
__global__ __launch_bounds__(MAXT, MINW) void ladder_colour_kernel(const LadderArgs a)
{
    constexpr bool STATS = false, SHORT = false;
#include "ladder_colour_body.inc"
}

// The same program with the swap and per-rung error counters of qecmc_plan_set_stats (choose_colour's colour_stats_key): fixed-length runs.  A wave
// is a slot here too: it counts the steps in which the pair below its slot traded states and sums the error counts its slot ends the steps with --
// two scalars of the wave, written once behind the step loop.
template <int CODE, int RULE>
__global__ __launch_bounds__(1024, 4) void ladder_colour_stats_kernel(const LadderArgs a)
{
    constexpr bool STATS = true, CONV = false, SHORT = false;
#include "ladder_colour_body.inc"
}

// The alpha rule's criterion kernel with the shortest-chain statistics of qecmc_plan_set_shortest (choose_shortest's colour_short_key); conv_mode NONE runs
// it to the horizon
template <int CODE>
__global__ __launch_bounds__(1024, 4) void ladder_colour_shortest_kernel(const LadderArgs a)
{
    constexpr bool STATS = false, CONV = true, SHORT = true;
    constexpr int RULE = 2;
#include "ladder_colour_body.inc"
}

}  // namespace qecmc
