// scan = 3 (QECMC_SCAN_WAVE): the reference's random-scan chain with a generator pick that the 64 ladders of a wavefront SHARE.
//
// Chain.update_chain (src/mcmc.py:19-43) picks a stabilizer generator uniformly and independently of the state
// (toric_model.py:287-296), and the ladders of different syndromes never interact.  So the 64 ladders a wavefront runs may all
// test the SAME generator at proposal k while every ladder keeps its own acceptance uniform: each ladder's chain has exactly the
// reference's law, only the noise of different syndromes becomes correlated.  What that buys on CDNA4:
//   * the four sites of a proposal are wave-uniform: word index and bit shift are scalars, so every rung's qubit_matrix can live
//     in REGISTERS (2 bits per qubit, W dwords per lane) and be addressed with the VGPR index mode (s_set_gpr_idx_on): one
//     VALU instruction reads a site (shift by a scalar, SDWA byte placement) and one updates it (v_xor under the accept mask);
//     no LDS traffic, no per-lane table gathers, no address arithmetic in the proposal loop;
//     the toric code packs its two layers interleaved (the wave layout, tables.hpp wave_position): the two qubits of a generator's own cell
//     share a word, three index switches per read and per update instead of four, a 32-byte descriptor (wu_read_cell, wu_xor_cell);
//     only the staging (wu_stage_lds) and the write_states epilogue know where a qubit sits;
//   * dE from the four old fields by one v_perm_b32 (a four-entry table per Pauli, applied to the four bytes at once) and one
//     v_sad_u8, which also adds the rung's threshold-row address: 4 (dE + 4) + base in a single instruction;
//   * the pick costs one Philox block per TWO proposals per wavefront (lane l draws the block of proposals 2l, 2l + 1 of a
//     window of up to 128 proposals), the per-ladder acceptance uniform 12 bits: one block per TEN proposals per lane; the 44-bit
//     uniform is completed (a 32-bit refinement word) only when a lane's 12 bits tie with its threshold's;
//   * the top rung (p = 0.75: every move is accepted, mcmc.py:30) applies its stabilizers blindly and collects its logical
//     operators -- wave-uniform now -- in one frame that is applied once per step.  The lean kernels with iters = 10 build all ten moves
//     of a step as one frame when the pick window is drawn (wu_frames.hpp): a step of the top rung's wave is one row read and the flush.
// States move through LDS once per ladder step, when the swap sweep (mcmc.py:94-103) has decided who goes where: every wave
// writes its rung's W words, and after the cascade reads the W words of the rung whose state it receives.
//
// RNG addressing of scan = 3 (the CPU oracle restates it independently, as its scan = 3): by ladder step T and proposal j of the step
// (1 <= iters <= 128), slot c:
//   pick      S = 128 / iters steps share a window: w = T / S, P = (T % S) iters + j; words A, B = 2 (P & 1), 2 (P & 1) + 1 of block
//             (64 w + (P >> 1), sub 9) with ctr[2] = (global ladder index) >> 6 and stream 0x800 + c -- lane P >> 1 of the wavefront draws
//             it --:  g = floor(B G / 2^32); top rung: logical iff A[31:16] < ceil(p_logical 2^16), its fields cut from A[15:0] and B as
//             in the packed layout of scan = 0 (philox.hpp)
//   accept    ten proposals share block (T ceil(iters / 10) + j / 10, sub 10) of the ladder's own index, stream c: a12 = field j % 10
//             (wu_field below); w32 = word j & 3 of block (T ceil(iters / 4) + (j >> 2), sub 11);
//             accept iff a12 2^32 + w32 < ceil(f^dE 2^44)
//   swaps     as in the other scans (block (T, i >> 2) of stream 0x100)
// Batches must start on a multiple of 64 (first_syndrome & 63 == 0) so that a wavefront is one pick group.
#pragma once
#include "ladder_kernel.hpp"
#include "shortest_book.hpp"
#include "wu_bounds.hpp"
#include "wu_frames.hpp"

namespace qecmc {

constexpr uint32_t kWuPickStream = 0x800u;
constexpr uint32_t kSubWuPick = 9u, kSubWuAcc = 10u, kSubWuRefine = 11u;

// Co-resident workgroups.  The issue arbiter serves the waves of a SIMD by priority, then by age, so on a one-round grid the
// oldest workgroup of a CU runs ahead and the youngest ends the launch alone, latency-bound (set_step_priority, pteq_book.hpp, is the same cure
// in ladder_kernel).  Every wave of a workgroup, in either role, takes the priority 3 - ((t >> kWuPrioShift) & 3) of its workgroup's step t since
// launch: a workgroup that is ahead by less than four periods issues behind the ones it left.  Priority enters no value: results cannot move.
// -DQECMC_WU_PRIO_SHIFT=n builds another period (bench.py --library), a negative n the kernels without it.
#ifndef QECMC_WU_PRIO_SHIFT
#define QECMC_WU_PRIO_SHIFT 4
#endif
constexpr int kWuPrioShift = QECMC_WU_PRIO_SHIFT;
// the families of wu_run that take it, by same-box A/B runs of each (profiles/r12_wave_priority_ab.json): the kernels of up to 16 state words under
// the depolarizing rule.  The 32-word kernels (4 - 6 waves per SIMD, several rounds or two workgroups per CU) lost 2.7 % at config 3 and held at
// config 5, the alpha rule's lost 16 % on its route: both keep the parent's code, and with the alpha rule the shortest-chain kernels.
// Under the depolarizing rule the criterion and queue kernels gained as the fixed-length ones did (-11.9 % on the criterion route); its statistics
// kernels inherit it.
constexpr bool wu_prio_family(int WV, bool ALPHA) { return kWuPrioShift >= 0 && !ALPHA && WV <= 16; }
// s_setprio takes an immediate, so the four cases are code; they are taken on the first step of a period only, and the other steps pay the
// test: three scalar instructions.  One asm statement, one scratch SGPR: written as a C++ switch the same code moved the register allocation
// of kernels that sit at their SGPR budget (the criterion kernel of toric L = 9: 36 -> 40 B of scratch).
__device__ __forceinline__ void wu_step_priority(uint32_t t)
{
    constexpr uint32_t SH = kWuPrioShift < 0 ? 0u : (uint32_t)kWuPrioShift;
    uint32_t k;
    asm volatile("s_and_b32 %0, %1, %2\n\t"
                 "s_cmp_lg_u32 %0, 0\n\t"
                 "s_cbranch_scc1 4f\n\t"
                 "s_bfe_u32 %0, %1, %3\n\t"                  // k = (t >> SH) & 3: priority 3 - k
                 "s_cmp_lg_u32 %0, 0\n\t"
                 "s_cbranch_scc1 1f\n\t"
                 "s_setprio 3\n\t"
                 "s_branch 4f\n"
                 "1:\n\t"
                 "s_cmp_lg_u32 %0, 1\n\t"
                 "s_cbranch_scc1 2f\n\t"
                 "s_setprio 2\n\t"
                 "s_branch 4f\n"
                 "2:\n\t"
                 "s_cmp_lg_u32 %0, 2\n\t"
                 "s_cbranch_scc1 3f\n\t"
                 "s_setprio 1\n\t"
                 "s_branch 4f\n"
                 "3:\n\t"
                 "s_setprio 0\n"
                 "4:"
                 : "=&s"(k) : "s"(t), "n"((1u << SH) - 1u), "n"(SH | (2u << 16)) : "scc");
}

template <int WV> struct WuVec;
template <> struct WuVec<4> { typedef uint32_t type __attribute__((ext_vector_type(4))); };
template <> struct WuVec<8> { typedef uint32_t type __attribute__((ext_vector_type(8))); };
template <> struct WuVec<12> { typedef uint32_t type __attribute__((ext_vector_type(12))); };
template <> struct WuVec<16> { typedef uint32_t type __attribute__((ext_vector_type(16))); };
template <> struct WuVec<32> { typedef uint32_t type __attribute__((ext_vector_type(32))); };

// The state registers are PINNED (the index mode addresses v[base + M0]) -- WV dwords ending at v63 (64-VGPR kernels) or at v127 --
// and every access to them is an asm statement that names the pinned tuple as an operand: the compiler then keeps the value where
// it is (any C++-level element access makes it a value of its own that is copied in and out of the pinned registers around every
// statement).  An "i" operand gives the register number of a static element, v[%c[r]].
// (32 words -- toric L <= 16, the one-layer codes L <= 22 --: v48 .. v79 of an 80-VGPR kernel, 6 waves per SIMD)
template <int WV> constexpr int wu_base() { return WV == 32 ? 48 : 64 - WV; }
#define WU_BY_WV(M)                                                                                                            \
    if constexpr (WV == 4) { M("{v[60:63]}") } else if constexpr (WV == 8) { M("{v[56:63]}") }                                 \
    else if constexpr (WV == 12) { M("{v[52:63]}") } else if constexpr (WV == 16) { M("{v[48:63]}") }                          \
    else { static_assert(WV == 32, "state widths: 4, 8, 12, 16, 32 words"); M("{v[48:79]}") }
#define WU_EACH(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) \
                   M(16) M(17) M(18) M(19) M(20) M(21) M(22) M(23) M(24) M(25) M(26) M(27) M(28) M(29) M(30) M(31)

template <int WV> __device__ __forceinline__ void wu_def(typename WuVec<WV>::type &st)
{
#define M(PIN) asm volatile("" : "=" PIN(st));
    WU_BY_WV(M)
#undef M
}
// (the tuple is in its pinned registers here: a value that only passes through -- a join of two paths -- has no other place to be)
template <int WV> __device__ __forceinline__ void wu_pin(typename WuVec<WV>::type &st)
{
#define M(PIN) asm volatile("" : "+" PIN(st));
    WU_BY_WV(M)
#undef M
}
template <int WV, int w> __device__ __forceinline__ void wu_set(typename WuVec<WV>::type &st, uint32_t v)
{
#define M(PIN) asm volatile("v_mov_b32 v[%c[r]], %[v]" : "+" PIN(st) : [r] "i"(wu_base<WV>() + w), [v] "v"(v));
    WU_BY_WV(M)
#undef M
}
template <int WV, int w> __device__ __forceinline__ uint32_t wu_get(typename WuVec<WV>::type &st)
{
    uint32_t v;
#define M(PIN) asm volatile("v_mov_b32 %[v], v[%c[r]]" : [v] "=v"(v), "+" PIN(st) : [r] "i"(wu_base<WV>() + w));
    WU_BY_WV(M)
#undef M
    return v;
}
// word w ^= m (m wave-uniform)
template <int WV, int w> __device__ __forceinline__ void wu_xor_s(typename WuVec<WV>::type &st, uint32_t m)
{
#define M(PIN) asm volatile("v_xor_b32 v[%c[r]], %[m], v[%c[r]]" : "+" PIN(st) : [r] "i"(wu_base<WV>() + w), [m] "s"(m));
    WU_BY_WV(M)
#undef M
}
// acc += number of non-identity fields of word w (toric_model.py:174-176 on the packed word)
template <int WV, int w> __device__ __forceinline__ void wu_count(typename WuVec<WV>::type &st, uint32_t &acc, uint32_t m55)
{
    uint32_t t;
#define M(PIN)                                                                                                                 \
    asm volatile("v_lshrrev_b32 %[t], 1, v[%c[r]]\n\t"                                                                         \
                 "v_bitop3_b32 %[t], %[t], v[%c[r]], %[m] bitop3:0xa8\n\t"                                                     \
                 "v_bcnt_u32_b32 %[acc], %[t], %[acc]"                                                                         \
                 : [t] "=&v"(t), [acc] "+v"(acc), "+" PIN(st) : [r] "i"(wu_base<WV>() + w), [m] "s"(m55));
    WU_BY_WV(M)
#undef M
}
// (row: the word's row of the rung's region in the exchange buffer -- w itself, or w - 16 for the upper half of a 32-word state, which
// passes through the buffer in two halves)
template <int WV, int w, int row = w> __device__ __forceinline__ void wu_ds_write(typename WuVec<WV>::type &st, uint32_t addr)
{
#define M(PIN) asm volatile("ds_write_b32 %[a], v[%c[r]] offset:%c[o]" : "+" PIN(st) : [a] "v"(addr), [r] "i"(wu_base<WV>() + w), [o] "i"(row * 256) : "memory");
    WU_BY_WV(M)
#undef M
}
template <int WV, int w, int row = w> __device__ __forceinline__ void wu_ds_read(typename WuVec<WV>::type &st, uint32_t addr)
{
#define M(PIN) asm volatile("ds_read_b32 v[%c[r]], %[a] offset:%c[o]" : "+" PIN(st) : [a] "v"(addr), [r] "i"(wu_base<WV>() + w), [o] "i"(row * 256) : "memory");
    WU_BY_WV(M)
#undef M
}
// (behind stores alone: nothing the tuple receives is waited for, so the statement does not name it and may stand inside a branch -- see the lean tail)
__device__ __forceinline__ void wu_ds_drain() { asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory"); }
template <int WV> __device__ __forceinline__ void wu_ds_wait(typename WuVec<WV>::type &st)
{
#define M(PIN) asm volatile("s_waitcnt lgkmcnt(0)" : "+" PIN(st) : : "memory");
    WU_BY_WV(M)
#undef M
}
// the whole state to / from a rung's region of the exchange buffer (row w: word w) as ONE asm statement of WV instructions -- between two asm
// statements that name the pinned tuple the compiler places a hazard s_nop, eleven per transfer at 12 words; the read waits for its data itself
#define WU_ROWS4(M) M(0, 0) M(1, 256) M(2, 512) M(3, 768)
#define WU_ROWS8(M) WU_ROWS4(M) M(4, 1024) M(5, 1280) M(6, 1536) M(7, 1792)
#define WU_ROWS12(M) WU_ROWS8(M) M(8, 2048) M(9, 2304) M(10, 2560) M(11, 2816)
#define WU_ROWS16(M) WU_ROWS12(M) M(12, 3072) M(13, 3328) M(14, 3584) M(15, 3840)
#define WU_PUT1(w, off) "ds_write_b32 %[a], v[%c[b]+" #w "] offset:" #off "\n\t"
#define WU_TAKE1(w, off) "ds_read_b32 v[%c[b]+" #w "], %[a] offset:" #off "\n\t"
template <int WV> __device__ __forceinline__ void wu_put_all(typename WuVec<WV>::type &st, uint32_t addr)
{
    static_assert(WV <= 16, "a 32-word state passes through the buffer in two halves");
#define M(ROWS, PIN) asm volatile(ROWS(WU_PUT1) : "+" PIN(st) : [a] "v"(addr), [b] "i"(wu_base<WV>()) : "memory");
    if constexpr (WV == 4) { M(WU_ROWS4, "{v[60:63]}") } else if constexpr (WV == 8) { M(WU_ROWS8, "{v[56:63]}") }
    else if constexpr (WV == 12) { M(WU_ROWS12, "{v[52:63]}") } else { M(WU_ROWS16, "{v[48:63]}") }
#undef M
}
template <int WV> __device__ __forceinline__ void wu_take_all(typename WuVec<WV>::type &st, uint32_t addr)
{
    static_assert(WV <= 16, "a 32-word state passes through the buffer in two halves");
#define M(ROWS, PIN) asm volatile(ROWS(WU_TAKE1) "s_waitcnt lgkmcnt(0)" : "+" PIN(st) : [a] "v"(addr), [b] "i"(wu_base<WV>()) : "memory");
    if constexpr (WV == 4) { M(WU_ROWS4, "{v[60:63]}") } else if constexpr (WV == 8) { M(WU_ROWS8, "{v[56:63]}") }
    else if constexpr (WV == 12) { M(WU_ROWS12, "{v[52:63]}") } else { M(WU_ROWS16, "{v[48:63]}") }
#undef M
}
// the four old fields of a generator's sites, one per byte of F (junk above bit 1 of every byte): site i sits in word d_i[7:0]
// at bit d_i[12:8]
template <int WV>
__device__ __forceinline__ uint32_t wu_read(typename WuVec<WV>::type &st, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3)
{
    uint32_t F;
#define M(PIN)                                                                                                                 \
    asm volatile("s_set_gpr_idx_on %[d0], 0x2\n\t"                                                                             \
                 "v_lshrrev_b32_sdwa %[F], %[d0], v[%c[b]] dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD\n\t"      \
                 "s_set_gpr_idx_idx %[d1]\n\t"                                                                                 \
                 "v_lshrrev_b32_sdwa %[F], %[d1], v[%c[b]] dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1 src1_sel:DWORD\n\t" \
                 "s_set_gpr_idx_idx %[d2]\n\t"                                                                                 \
                 "v_lshrrev_b32_sdwa %[F], %[d2], v[%c[b]] dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1 src1_sel:DWORD\n\t" \
                 "s_set_gpr_idx_idx %[d3]\n\t"                                                                                 \
                 "v_lshrrev_b32_sdwa %[F], %[d3], v[%c[b]] dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1 src1_sel:DWORD\n\t" \
                 "s_set_gpr_idx_off"                                                                                           \
                 : [F] "=&v"(F), "+" PIN(st)                                                                                   \
                 : [d0] "s"(d0), [d1] "s"(d1), [d2] "s"(d2), [d3] "s"(d3), [b] "i"(wu_base<WV>()));
    WU_BY_WV(M)
#undef M
    return F;
}
// the accepted move: word d_i[7:0] ^= x_i (under the caller's exec mask; sites may share a word: four read-modify-writes in order)
template <int WV>
__device__ __forceinline__ void wu_xor(typename WuVec<WV>::type &st, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3,
                                       uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3)
{
#define M(PIN)                                                                                                                 \
    asm volatile("s_set_gpr_idx_on %[d0], 0xA\n\t"                                                                             \
                 "v_xor_b32 v[%c[b]], %[x0], v[%c[b]]\n\t"                                                                     \
                 "s_set_gpr_idx_idx %[d1]\n\t"                                                                                 \
                 "v_xor_b32 v[%c[b]], %[x1], v[%c[b]]\n\t"                                                                     \
                 "s_set_gpr_idx_idx %[d2]\n\t"                                                                                 \
                 "v_xor_b32 v[%c[b]], %[x2], v[%c[b]]\n\t"                                                                     \
                 "s_set_gpr_idx_idx %[d3]\n\t"                                                                                 \
                 "v_xor_b32 v[%c[b]], %[x3], v[%c[b]]\n\t"                                                                     \
                 "s_set_gpr_idx_off"                                                                                           \
                 : "+" PIN(st)                                                                                                 \
                 : [d0] "s"(d0), [d1] "s"(d1), [d2] "s"(d2), [d3] "s"(d3), [x0] "s"(x0), [x1] "s"(x1), [x2] "s"(x2), [x3] "s"(x3),  \
                   [b] "i"(wu_base<WV>()));
    WU_BY_WV(M)
#undef M
}
// The toric code's forms (the wave layout, tables.hpp toric_wave_descriptors): sites 0 and 1 -- the generator's own cell -- are adjacent fields of
// ONE word, d01 = word | s << 8 | (s + 2) << 16, so a read switches the index three times instead of four ...
template <int WV>
__device__ __forceinline__ uint32_t wu_read_cell(typename WuVec<WV>::type &st, uint32_t d01, uint32_t d2, uint32_t d3)
{
    uint32_t F;
#define M(PIN)                                                                                                                 \
    asm volatile("s_set_gpr_idx_on %[d01], 0x2\n\t"                                                                            \
                 "v_lshrrev_b32_sdwa %[F], %[d01], v[%c[b]] dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD\n\t"      \
                 "v_lshrrev_b32_sdwa %[F], %[d01], v[%c[b]] dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_2 src1_sel:DWORD\n\t" \
                 "s_set_gpr_idx_idx %[d2]\n\t"                                                                                 \
                 "v_lshrrev_b32_sdwa %[F], %[d2], v[%c[b]] dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1 src1_sel:DWORD\n\t" \
                 "s_set_gpr_idx_idx %[d3]\n\t"                                                                                 \
                 "v_lshrrev_b32_sdwa %[F], %[d3], v[%c[b]] dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1 src1_sel:DWORD\n\t" \
                 "s_set_gpr_idx_off"                                                                                           \
                 : [F] "=&v"(F), "+" PIN(st)                                                                                   \
                 : [d01] "s"(d01), [d2] "s"(d2), [d3] "s"(d3), [b] "i"(wu_base<WV>()));
    WU_BY_WV(M)
#undef M
    return F;
}
// ... and the accepted move is three read-modify-writes, the pair's with one value (5 P << s)
template <int WV>
__device__ __forceinline__ void wu_xor_cell(typename WuVec<WV>::type &st, uint32_t d01, uint32_t d2, uint32_t d3, uint32_t x01, uint32_t x2, uint32_t x3)
{
#define M(PIN)                                                                                                                 \
    asm volatile("s_set_gpr_idx_on %[d01], 0xA\n\t"                                                                            \
                 "v_xor_b32 v[%c[b]], %[x01], v[%c[b]]\n\t"                                                                    \
                 "s_set_gpr_idx_idx %[d2]\n\t"                                                                                 \
                 "v_xor_b32 v[%c[b]], %[x2], v[%c[b]]\n\t"                                                                     \
                 "s_set_gpr_idx_idx %[d3]\n\t"                                                                                 \
                 "v_xor_b32 v[%c[b]], %[x3], v[%c[b]]\n\t"                                                                     \
                 "s_set_gpr_idx_off"                                                                                           \
                 : "+" PIN(st)                                                                                                 \
                 : [d01] "s"(d01), [d2] "s"(d2), [d3] "s"(d3), [x01] "s"(x01), [x2] "s"(x2), [x3] "s"(x3), [b] "i"(wu_base<WV>()));
    WU_BY_WV(M)
#undef M
}
// a toric descriptor: 32 bytes, one scalar load
typedef uint32_t wu_desc8 __attribute__((ext_vector_type(8)));
typedef const wu_desc8 __attribute__((address_space(4))) *wu_const_desc8;

// (the LDS carve-up of one workgroup, wu_lds, and the padded state width wu_words: kernel_choice.hpp)
__host__ __device__ inline int wu_words_min(int WV) { return WV == 4 ? 1 : WV == 32 ? 17 : WV - 3; }      // the narrowest W a WV-word kernel serves

// A Philox block whose key schedule is formed where it is used (two scalar adds per round) instead of being hoisted out of the
// step loop into twenty scalar registers per call site: the kernel runs at 8 waves per SIMD on ~80 SGPRs.
__device__ __forceinline__ u32x4 wu_philox(uint64_t k, uint32_t sub, uint32_t syndrome, uint32_t stream, uint32_t seed_lo, uint32_t seed_hi)
{
    asm volatile("" : "+s"(seed_lo), "+s"(seed_hi));
    return philox_block(k, sub, syndrome, stream, seed_lo, seed_hi);
}

typedef const uint32_t __attribute__((address_space(4))) *wu_const_ptr;
typedef const uint32_t __attribute__((address_space(3))) *wu_lds_ptr;
typedef uint32_t __attribute__((address_space(3))) *wu_lds_rw;

constexpr uint32_t kWuDead = 0xFFFFFFFFu, kWuKeep = 0xFFFFFFFEu;      // refill mailbox: no ladder left for the lane / the lane keeps its ladder

struct WuCtx {
    uint32_t n4, cls, flag, tops0, samples, done, conv_ok, steps_done, nef;
    uint32_t swapc = 0, nsum = 0;      // STATS: the steps in which the pair below this wave's slot traded states, the summed error counts the slot held
};
struct WuEnv {
    uint32_t lds0, thr_off, lml_off, cht_off, frm_off, slot, grp, lad;    // frm_off: the top rung's frames (wu_frames.hpp); lad: the lane's first ladder of this launch (kWuDead: none)
    int lane;
    uint64_t chunk_hi;                                  // QUEUE: end of the workgroup's share of the batch
};

// field f (0 .. 9) of an acceptance block: twelve leading bits of a 44-bit uniform each -- two per word in bits 0-23, the last two
// gathered from the four top bytes
__device__ __forceinline__ uint32_t wu_field(const u32x4 &b, int f)
{
    if (f < 8) {
        const uint32_t w = sel4(b, f >> 1);
        return (f & 1) ? __builtin_amdgcn_ubfe(w, 12u, 12u) : (w & 0xFFFu);
    }
    const uint32_t lo = f == 8 ? b.x : b.z, hi = f == 8 ? b.y : b.w;
    return __builtin_amdgcn_perm(hi, lo, 0x0C0C0703u) & 0xFFFu;      // byte 3 of lo | byte 3 of hi << 8
}

// one Metropolis proposal of a rung below the top (mcmc.py:38-42) on the 64 ladders of the wave: the generator of descriptor e[0..11] (toric: e[0..6]),
// a12 = the lanes' leading acceptance bits.  The 12 bits decide unless they tie with the threshold's in some lane (once in 4096 per lane).
// (toric: d0 is the own-cell pair's dword and x0 its value, d1 and x1 are unused)
template <int CODE, int WV>
__device__ __forceinline__ void wu_propose(typename WuVec<WV>::type &st, uint32_t &n4, uint32_t a12, uint32_t thr_base, uint32_t nbias,
                                           uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3,
                                           uint32_t tlo, uint32_t thi, uint32_t omask, uint32_t amask,
                                           uint64_t refine_k, uint32_t refine_w, uint32_t syn, uint32_t slot, uint32_t seed_lo, uint32_t seed_hi)
{
    uint32_t F;
    if constexpr (CODE == kCodeToric) F = wu_read_cell<WV>(st, d0, d2, d3);
    else F = wu_read<WV>(st, d0, d1, d2, d3);
    uint32_t pv;
    if constexpr (CODE == kCodeToric) pv = __builtin_amdgcn_perm(tlo, tlo, F & 0x03030303u);   // byte i: 4 (1 + change of the error count at site i)
    else pv = __builtin_amdgcn_perm(thi, tlo, (F & amask) | omask);                            // (null sites and the second Pauli's half of the table)
    const uint32_t addr = __builtin_amdgcn_sad_u8(pv, 0u, thr_base);                           // LDS address of this rung's threshold for dE
    const uint32_t Th = *(wu_lds_ptr)(uintptr_t)addr;
    bool acc = a12 < Th;
    if (__builtin_amdgcn_uicmp(a12, Th, 32) != 0) {
        const u32x4 rb = wu_philox(refine_k, kSubWuRefine, syn, slot, seed_lo, seed_hi);
        const uint32_t Tl = *(wu_lds_ptr)(uintptr_t)(addr + 36u);
        if (a12 == Th) acc = sel4(rb, (int)refine_w) < Tl;
    }
    if (acc) {
        if constexpr (CODE == kCodeToric) wu_xor_cell<WV>(st, d0, d2, d3, x0, x2, x3);
        else wu_xor<WV>(st, d0, d1, d2, d3, x0, x1, x2, x3);
        n4 = n4 + addr + nbias;                                                                 // n += dE
    }
}

// ---- the alpha rule (src/mcmc_alpha.py) -----------------------------------------------------------------------------------------
typedef _Float16 wu_half2 __attribute__((ext_vector_type(2)));
typedef const double __attribute__((address_space(3))) *wu_lds_dptr;
typedef double __attribute__((address_space(3))) *wu_lds_drw;

// nx / nz / nxy += the fields of word w that are 1 / 3 / 1 or 2 (Chain_alpha.__init__, mcmc_alpha.py:18-22, on the packed word)
template <int WV, int w> __device__ __forceinline__ void wu_count3(typename WuVec<WV>::type &st, uint32_t &nx, uint32_t &nz, uint32_t &nxy, uint32_t m55)
{
    uint32_t t, u;
#define M(PIN)                                                                                                                 \
    asm volatile("v_lshrrev_b32 %[t], 1, v[%c[r]]\n\t"                                                                         \
                 "v_bitop3_b32 %[u], %[t], v[%c[r]], %[m] bitop3:0x08\n\t"                                                     \
                 "v_bcnt_u32_b32 %[nx], %[u], %[nx]\n\t"                                                                       \
                 "v_bitop3_b32 %[u], %[t], v[%c[r]], %[m] bitop3:0x80\n\t"                                                     \
                 "v_bcnt_u32_b32 %[nz], %[u], %[nz]\n\t"                                                                       \
                 "v_bitop3_b32 %[u], %[t], v[%c[r]], %[m] bitop3:0x28\n\t"                                                     \
                 "v_bcnt_u32_b32 %[nxy], %[u], %[nxy]"                                                                         \
                 : [t] "=&v"(t), [u] "=&v"(u), [nx] "+v"(nx), [nz] "+v"(nz), [nxy] "+v"(nxy), "+" PIN(st)                      \
                 : [r] "i"(wu_base<WV>() + w), [m] "s"(m55));
    WU_BY_WV(M)
#undef M
}
template <int WV, int w> __device__ __forceinline__ void wu_count_x(typename WuVec<WV>::type &st, uint32_t &nx, uint32_t m55)
{
    uint32_t t;
#define M(PIN)                                                                                                                 \
    asm volatile("v_lshrrev_b32 %[t], 1, v[%c[r]]\n\t"                                                                         \
                 "v_bitop3_b32 %[t], %[t], v[%c[r]], %[m] bitop3:0x08\n\t"                                                     \
                 "v_bcnt_u32_b32 %[nx], %[t], %[nx]"                                                                           \
                 : [t] "=&v"(t), [nx] "+v"(nx), "+" PIN(st) : [r] "i"(wu_base<WV>() + w), [m] "s"(m55));
    WU_BY_WV(M)
#undef M
}
// the state's counts, packed n_x | n_z << 10 | (n_x + n_y) << 20
// (W: the words in use -- wave-uniform; the padding words of a WV-word kernel are zero and need not be looked at)
template <int WV> __device__ __forceinline__ uint32_t wu_counts_packed(typename WuVec<WV>::type &st, uint32_t m55, int W = WV)
{
    uint32_t nx = 0, nz = 0, nxy = 0;
#define QECMC_WU_C3(w) if constexpr (w < WV) { if (w < wu_words_min(WV) || w < W) wu_count3<WV, w>(st, nx, nz, nxy, m55); }
    WU_EACH(QECMC_WU_C3)
#undef QECMC_WU_C3
    return nx | (nz << 10) | (nxy << 20);
}
// Ladder_alpha.r_flip (mcmc_alpha.py:118-123) on the slots' attributes: u < (pz_lo / pz_hi) ** (n_eff_hi - n_eff_lo), the power as
// det_exp(e ln b) like the CPU oracle -- behind a single-precision estimate of 2^32 times it that settles all but ~6e-5 of the tests
// (the estimate's relative error stays below 5e-6: the exponent is rounded to a float of magnitude <= 32 wherever the outcome is open)
__device__ __forceinline__ bool wu_alpha_flip(uint32_t x, double ne_hi, double ne_lo, double lnb)
{
#pragma clang fp contract(off)
    const double e = ne_hi - ne_lo;
    const double y = e * lnb;
    if (!(y < 0.0)) return true;                                       // (det_exp returns 1: every u passes)
    const float ef = __builtin_amdgcn_exp2f(__builtin_fmaf((float)y, 1.44269504f, 32.0f));
    const float xf = (float)x, band = __builtin_fmaf(ef, 3.0e-5f, 2.0f);
    if (xf < ef - band) return true;
    if (xf > ef + band) return false;
    return (double)x * (1.0 / 4294967296.0) < det_exp(y);
}

struct WuAl { uint32_t Dh, any, Nb; };     // the counts' change since the step began (D_xy | D_z << 16, fp16 integers), "a move was accepted", the counts then

// one proposal of a rung below the top under the alpha rule (mcmc_alpha.py:61-70): accept iff u < p_n / p_b with p_b frozen when the step
// began (Q3).  log2 of the ratio is lxy D_xy + lz D_z with D the count change since then, so two fmas and a v_exp_f32 give 2^12 p_n / p_b to
// well within a unit (the plan has checked 4 iters max|l| <= 2000: ladder_kernel.hpp, the same estimate), and only a lane whose twelve
// leading uniform bits lie within a cell or two of it evaluates the reference's expression -- on the power tables, in its order.
template <int CODE, int WV>
__device__ __forceinline__ void wu_propose_alpha(const LadderArgs &a, typename WuVec<WV>::type &st, WuAl &al, uint32_t a12, uint32_t cht_addr,
                                                 float lxy, float lz, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3,
                                                 uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t tlo, uint32_t thi, uint32_t omask, uint32_t amask,
                                                 uint64_t refine_k, uint32_t refine_w, uint32_t syn, uint32_t slot, uint32_t m55)
{
    const uint32_t F = wu_read<WV>(st, d0, d1, d2, d3);
    const uint32_t pv = __builtin_amdgcn_perm(thi, tlo, (F & amask) | omask);      // byte i: 4 ((dz + 1) + 9 (dxy + 1)) of site i (a missing site: 0)
    const uint32_t addr = __builtin_amdgcn_sad_u8(pv, 0u, cht_addr);               // LDS address of the proposal's (D_xy, D_z)
    const uint32_t dch = *(wu_lds_ptr)(uintptr_t)addr;
    const wu_half2 pD = __builtin_bit_cast(wu_half2, al.Dh) + __builtin_bit_cast(wu_half2, dch);
    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf((float)pD.x, lxy, __builtin_fmaf((float)pD.y, lz, 12.0f)));
    const float dm = e - (float)a12;
    bool acc = dm >= 2.0f;
    if (!acc && dm >= -1.0f) {
        // the reference's expression (mcmc_alpha.py:64-68): counts of the proposal and of the state the step began with
        const int nq = a.nq, T1 = nq + 1;
        const double *bt = a.bias_tbl + (size_t)slot * 4 * T1;
        uint32_t nxc = 0;
#define QECMC_WU_CX(w) if constexpr (w < WV) wu_count_x<WV, w>(st, nxc, m55);
        WU_EACH(QECMC_WU_CX)
#undef QECMC_WU_CX
        int dx = 0;
        {
            const uint32_t P0 = x0 >> ((d0 >> 8) & 31u), P1 = x1 >> ((d1 >> 8) & 31u), P2 = x2 >> ((d2 >> 8) & 31u), P3 = x3 >> ((d3 >> 8) & 31u);
            const uint32_t f0 = F & 3u, f1 = (F >> 8) & 3u, f2 = (F >> 16) & 3u, f3 = (F >> 24) & 3u;
            dx += (int)((f0 ^ P0) == 1u) - (int)(f0 == 1u);
            dx += (int)((f1 ^ P1) == 1u) - (int)(f1 == 1u);
            dx += (int)((f2 ^ P2) == 1u) - (int)(f2 == 1u);
            dx += (int)((f3 ^ P3) == 1u) - (int)(f3 == 1u);
        }
        const int bx = (int)(al.Nb & 1023u), bz = (int)((al.Nb >> 10) & 1023u), bxy = (int)(al.Nb >> 20);
        const int cx = (int)nxc + dx, cz = bz + (int)(float)pD.y, cxy = bxy + (int)(float)pD.x;
        const double pn = bt[cx] * bt[T1 + (cxy - cx)] * bt[2 * T1 + cz] * bt[3 * T1 + (nq - cxy - cz)];
        const double pb = bt[bx] * bt[T1 + (bxy - bx)] * bt[2 * T1 + bz] * bt[3 * T1 + (nq - bxy - bz)];
        const double ratio = pn / pb;
        const double ulo = (double)a12 * (1.0 / 4096.0);
        acc = ulo + (1.0 / 4096.0) <= ratio;
        if (!acc && ulo < ratio) {
            const u32x4 rb = wu_philox(refine_k, kSubWuRefine, syn, slot, a.seed_lo, a.seed_hi);
            const uint64_t v44 = ((uint64_t)a12 << 32) | sel4(rb, (int)refine_w);
            acc = (double)v44 * (1.0 / 17592186044416.0) < ratio;
        }
    }
    if (acc) {
        wu_xor<WV>(st, d0, d1, d2, d3, x0, x1, x2, x3);
        al.Dh = __builtin_bit_cast(uint32_t, pD);
        al.any = 1u;
    }
}

// this rung's seed configuration of ladder `lad`, packed 2 bits per qubit, into the lane's column of the rung's rows of the exchange
// buffer (Ladder.__init__ copies the seed into every rung, mcmc.py:72; resume: the rung's own state) -- a short runtime loop; the caller
// then takes the words into its state registers with the exchange's own static reads.  Returns 4 x the error count and the class.
// (a 32-word kernel stages words [w0, w1) = [0, 16) and [16, W) in two calls, each into rows 0 .. of the rung's region; the class comes with the first)
template <int CODE>
// (rows: the rows of the region to fill -- those beyond the words of the range get zeros: the padding words of the state)
__device__ __forceinline__ void wu_stage_lds(const LadderArgs &a, uint64_t lad, uint32_t slot, wu_lds_rw xrow, uint32_t &n4, uint32_t &cls, int w0 = 0, int w1 = -1, int rows = 0)
{
    const int NC = a.Nc, W = a.W, L = a.L, nq = a.nq;
    const uint8_t *src = a.resume ? a.states + (lad * NC + slot) * (uint64_t)nq : a.init + (lad / a.replicas) * (uint64_t)nq;
    uint32_t cnt = 0;
    if (w1 < 0) w1 = W;
#pragma unroll 1
    for (int w = w0; w < w1; ++w) {
        uint32_t word = 0;
#pragma unroll 4
        for (int b = 0; b < 16; ++b) {
            // (the wave layout, tables.hpp wave_position -- toric: field b of word w is layer b & 1 of cell 8 w + (b >> 1))
            const int cell = w * 8 + (b >> 1), q = CODE == kCodeToric ? (cell < L * L ? (b & 1) * L * L + cell : nq) : w * 16 + b;
            if (q < nq) word |= (uint32_t)(src[q] & 3u) << (2 * b);
        }
        xrow[(w - w0) * 64] = word;
        cnt += nnz2(word);
    }
#pragma unroll 1
    for (int r = w1 - w0; r < rows; ++r) xrow[r * 64] = 0u;
    if (w0 != 0) { n4 += 4u * cnt; return; }
    n4 = 4u * cnt;
    cls = (uint32_t)(CODE == kCodeToric ? toric_eq_class_b(L, src) : surf_eq_class_b(CODE, L, src));
    if (CODE == kCodeXzzx) cls = cls == 0 ? 0u : cls == 1 ? 1u : cls == 2 ? 3u : 2u;   // the internal value v with class = v ^ (v >> 1)
}

// The swap sweep (mcmc.py:97-99, _r_flip :146-149) under the depolarizing rule, lean tail: slots i and i + 1 trade states iff ne_hi - ne_lo <= D_i(x)
// (wu_bounds.hpp), and whoever draws a block of swap uniforms leaves the bounds in their place, in front of the step's first barrier.  v: the block's four
// words, of pairs i0 .. i0 + 3 (`left` of them exist); trow: LDS byte address of pair i0's row of swapT.  Every word's guess is checked on two adjacent
// entries of its row -- one read, no branch, the four independent of each other --, and one test the wave shares sends the lanes whose check failed
// somewhere (a quotient within rounding of an integer, x = 0, 1, 2, ladders kSwapFast apart: about one step in a hundred) through the table walk, which
// leaves the row for the plan's table in global memory -- whose entries fit 32 bits: swap_fast_ok, wu_supported().  The cascade then reads no
// table and has no far path: a subtraction and a compare per pair.
__device__ __forceinline__ void wu_bound_block(const LadderArgs &a, u32x4 &v, uint32_t trow, int i0, int left)
{
    int nql = a.nq;
    asm volatile("" : "+s"(nql));
    constexpr uint32_t RB = (uint32_t)(kSwapFast * 4);
    auto near = [&](uint32_t row) { return [row](int d) { return *(wu_lds_ptr)(uintptr_t)(row + 4u * (uint32_t)d); }; };
    uint32_t g0 = 0, g1 = 0, g2 = 0, g3 = 0;
    bool ok = true, ok1 = true, ok2 = true, ok3 = true;
    if (left > 2) {
        // (three or four pairs: all four words in one stretch, their reads in flight together -- the fourth, if its pair does not exist, on the idle last
        // row of swapT, its answer dropped)
        g0 = wu_swap_first(v.x, a.swap_inv_log2[i0], nql); g1 = wu_swap_first(v.y, a.swap_inv_log2[i0 + 1], nql);
        g2 = wu_swap_first(v.z, a.swap_inv_log2[i0 + 2], nql); g3 = wu_swap_first(v.w, a.swap_inv_log2[i0 + 3], nql);
        uint32_t a0 = near(trow)((int)g0), b0 = near(trow)((int)g0 + 1), a1 = near(trow + RB)((int)g1), b1 = near(trow + RB)((int)g1 + 1);
        uint32_t a2 = near(trow + 2u * RB)((int)g2), b2 = near(trow + 2u * RB)((int)g2 + 1), a3 = near(trow + 3u * RB)((int)g3), b3 = near(trow + 3u * RB)((int)g3 + 1);
        asm volatile("" : "+v"(a0), "+v"(b0), "+v"(a1), "+v"(b1), "+v"(a2), "+v"(b2), "+v"(a3), "+v"(b3));      // (all eight here: one wait)
        ok = wu_swap_holds(v.x, a0, b0); ok1 = wu_swap_holds(v.y, a1, b1); ok2 = wu_swap_holds(v.z, a2, b2);
        ok3 = left == 3 || wu_swap_holds(v.w, a3, b3);
    } else {
        ok = wu_swap_guess(v.x, a.swap_inv_log2[i0], nql, near(trow), g0);
        if (left > 1) ok1 = wu_swap_guess(v.y, a.swap_inv_log2[i0 + 1], nql, near(trow + RB), g1);
    }
    if (__builtin_amdgcn_ballot_w64(!(ok && ok1 && ok2 && ok3)) != 0) {
        int il = i0;
        asm volatile("" : "+s"(il));
        auto far = [&](int k) { return [&a, il, nql, k](int d) { return (uint32_t)a.swap_thr[(size_t)(il + k) * (size_t)(nql + 1) + (size_t)d]; }; };
        if (!ok) g0 = wu_swap_walk(v.x, g0, nql, near(trow), far(0));
        if (!ok1) g1 = wu_swap_walk(v.y, g1, nql, near(trow + RB), far(1));
        if (!ok2) g2 = wu_swap_walk(v.z, g2, nql, near(trow + 2u * RB), far(2));
        if (!ok3) g3 = wu_swap_walk(v.w, g3, nql, near(trow + 3u * RB), far(3));
    }
    v.x = g0; v.y = g1; v.z = g2; v.w = g3;
}
// ... and of ONE word, for the form of the walk in which every wave below the top finds the bound of one pair (LadderArgs::wu_once == 2, below): x the raw
// swap word of pair i, trow the LDS byte address of that pair's row of swapT.  The same functions on the same inputs as a word of wu_bound_block.
__device__ __forceinline__ uint32_t wu_bound_word(const LadderArgs &a, uint32_t x, uint32_t trow, int i)
{
    int nql = a.nq;
    asm volatile("" : "+s"(nql));
    auto near = [trow](int d) { return *(wu_lds_ptr)(uintptr_t)(trow + 4u * (uint32_t)d); };
    uint32_t g;
    const bool ok = wu_swap_guess(x, a.swap_inv_log2[i], nql, near, g);
    if (__builtin_amdgcn_ballot_w64(!ok) != 0) {
        int il = i;
        asm volatile("" : "+s"(il));
        if (!ok) g = wu_swap_walk(x, g, nql, near, [&a, il, nql](int d) { return (uint32_t)a.swap_thr[(size_t)il * (size_t)(nql + 1) + (size_t)d]; });
    }
    return g;
}
// the words of a block of swap uniforms (or their bounds) into the rows of swd: p = row of the block's first pair, lane's column; `left` pairs exist from there
__device__ __forceinline__ void wu_put_block(wu_lds_rw p, const u32x4 &v, int left)
{
    p[0] = v.x;
    if (left > 1) p[64] = v.y;
    if (left > 2) p[128] = v.z;
    if (left > 3) p[192] = v.w;
}
// Where a wave below the top turns its pair's word into the bound under wu_once == 2: 0 right behind the exchange's read (the top of its stretch between the
// third barrier and the next step's first), 1 behind the proposals (the end of that stretch).  The results are the same; -DQECMC_WU_SPREAD_AT=n builds the
// other one for an A/B (bench.py --library; DESIGN.md 4.1g has the measurement that chose the default; the other build was timed, the tests run the default).
#ifndef QECMC_WU_SPREAD_AT
#define QECMC_WU_SPREAD_AT 0
#endif
constexpr int kWuSpreadAt = QECMC_WU_SPREAD_AT;
// The barriers of a step of the walked forms (wu_once 1, 2; the lean tail has the schedule and the access argument): 2 -- every wave publishes its record
// in FRONT of the step's first barrier, the top rung's wave walks right behind it and the state stores of every wave go into the walk's shadow --, 3 -- the
// parent's step: first barrier, stores and record, second barrier, walk, third barrier.  The replay (wu_once 0) has its two barriers in either build.
// -DQECMC_WU_STEP_BARRIERS=3 builds the other form for an A/B (bench.py --library; DESIGN.md 4.1g has the measurement; the tests run the default).
#ifndef QECMC_WU_STEP_BARRIERS
#define QECMC_WU_STEP_BARRIERS 2
#endif
constexpr int kWuStepBarriers = QECMC_WU_STEP_BARRIERS;
// (the walker's own state stores of the two-barrier step: 0 behind the walk's loads, in whose wait they are issued; 1 in front of them)
#ifndef QECMC_WU_WALK_PUTS_FIRST
#define QECMC_WU_WALK_PUTS_FIRST 0
#endif
constexpr bool kWuWalkPutsFirst = QECMC_WU_WALK_PUTS_FIRST != 0;
static_assert(kWuStepBarriers == 2 || kWuStepBarriers == 3, "a step of the walked forms: two or three barriers");
// Who books rung 0's new record (tops0, the class histogram, samples) in the walked forms: 0 -- the wave of slot 0, as in the replay --, 1 -- the top
// rung's wave, which ends its walk holding exactly that record.  By the static counts the walker has the workgroup's shortest stretch to the next step's
// first barrier and wave 0 the longest; measured, the walker's booking LOST 0.8 - 1.4 % at 5 .. 8 rungs, with either number of barriers (DESIGN.md 4.1g,
// profiles/r16_wave_two_barriers_ab.json), so 0 is the default and -DQECMC_WU_TOP_BOOKS=1 builds the other one (timed; the tests run the default).
#ifndef QECMC_WU_TOP_BOOKS
#define QECMC_WU_TOP_BOOKS 0
#endif
constexpr bool kWuTopBooks = QECMC_WU_TOP_BOOKS != 0;
// (the kernels whose lean tail can walk at all: what folds LadderArgs::wu_once to 0 in wu_run, for ladder_wu_body.inc's hand-over of the booked values)
constexpr bool wu_top_books_family(int WV, bool CONV, bool ALPHA, bool STATS, bool LONG) { return kWuTopBooks && !CONV && !ALPHA && WV <= 16 && !STATS && !LONG; }

// the step loop of one wave: TOP = the rung that accepts every move (its stabilizers unseen, its logical operators through a frame);
// IT = 10: `iters` known at compile time (decoders.py:25 iters=10), the proposal loop unrolled without guards; IT = 0: any 1 <= iters <= 128.
// QUEUE (with CONV): a persistent grid; a lane whose ladder has ended takes the next one of its workgroup's share of the batch (in lane
// order among the lanes that end together, so the assignment does not depend on timing): the acceptance and swap uniforms follow
// the ladder (its index, its own step), the generator picks the lane's position (group, workgroup step).
// ALPHA: the alpha noise model's ladder (src/mcmc_alpha.py; xzzx / rotated codes): wu_propose_alpha, slot-bound n_eff attributes (Q4) -- a wave IS
// a slot here, so its attribute is a register --, the floating-point swap test, the criterion on the logged count pairs.
// STATS (ladder_wu_stats_kernel): the equilibrium observables of qecmc_plan_set_stats.  The wave of slot s >= 1 itself decides pair s - 1 when it
// replays the cascade and ends the step holding its slot's record: two counters per lane, in registers (cx.swapc, cx.nsum), no LDS, no atomics.
// LONG: the ladder may have more than 8 rungs (the kernels under the launch bound of 1 024 threads): up to four blocks of swap uniforms, one per wave.
// SHORT (ladder_wu_shortest_kernel): the shortest-chain statistics of qecmc_plan_set_shortest (shortest_book.hpp) on the alpha rule's queue kernel, run with
// one ladder per lane (wu_chunk = 64: no refill).  Wave 0, which ends a step holding rung 0's new state in registers, leaves that state's 64-bit key beside
// bot / bot2; the booking wave, a step behind, applies the reference's rule to its lane's rows in LDS.  conv_mode NONE: the criterion is never consulted.
template <int CODE, int WV, bool CONV, bool QUEUE, bool TOP, int IT, bool ALPHA, bool STATS = false, bool SHORT = false, bool LONG = true>
__device__ __forceinline__ void wu_run(const LadderArgs &a, typename WuVec<WV>::type &st, WuCtx &cx, const WuEnv &ev)
{
    static_assert(!QUEUE || CONV, "the work queue serves the runs that stop by the criterion");
    static_assert(!ALPHA || CODE != kCodeToric, "the alpha rule: xzzx / rotated codes");
    static_assert(!STATS || (!CONV && WV <= 16), "the statistics kernels: fixed-length runs of up to 16 state words");
    static_assert(!SHORT || (CONV && QUEUE && ALPHA && !STATS), "the shortest-chain kernels: the alpha rule's queue kernels");
    [[maybe_unused]] uint32_t swapc = 0, nsum = 0;
    const int L = a.L;
    wu_lds_ptr const lml = (wu_lds_ptr)(uintptr_t)(ev.lds0 + ev.lml_off);
    const uint32_t lds0 = ev.lds0, slot = ev.slot, grp = ev.grp;
    const int lane = ev.lane;
    constexpr bool top = TOP;
    constexpr bool LEAN = !CONV && !ALPHA && WV <= 16;                            // the kernels whose step tail is the lean one below
    // the top rung's role of the lean kernels with the unrolled loop: its ten moves of a step are one row of frames built with the pick window
    // (wu_frames.hpp; the buffer: wu_lds's frm, private to this wave) -- no proposal loop, no picks held across steps
    constexpr bool FRAME = TOP && wu_frame_steps(WV, CONV, ALPHA, IT) != 0;
    constexpr uint32_t FW = (uint32_t)WV + 1u;                                    // words of a row: the mask of the WV state words, the class change
    const uint32_t G = a.n_gen;
    const uint32_t m55 = 0x55555555u;
    uint32_t n4 = cx.n4, cls = cx.cls, flag = cx.flag;
    [[maybe_unused]] uint32_t nef = cx.nef;                                       // ALPHA: this slot's n_eff attribute as n_z | (n_x + n_y) << 16
    [[maybe_unused]] float lxyf = 0.0f, lzf = 0.0f;
    if constexpr (ALPHA) { lxyf = a.bias_l2f[ev.slot][0]; lzf = a.bias_l2f[ev.slot][1]; }
    [[maybe_unused]] const uint32_t cht_base = ev.lds0 + ev.cht_off;
    uint32_t syn = a.first_syndrome + ev.lad;                                     // Philox ctr[2] of the lane's ladder
    [[maybe_unused]] uint32_t t0 = 0;                                             // QUEUE: the workgroup step the lane's ladder started at
    [[maybe_unused]] uint32_t tops0 = cx.tops0, samples = 0;                      // wave 0 of the fixed-length kernels: in registers
    const wu_const_ptr desc = (wu_const_ptr)a.wu_desc;
    const uint32_t iters = IT ? (uint32_t)IT : a.iters;
    const uint32_t nch = (iters + 9u) / 10u, nc4 = (iters + 3u) / 4u;             // acceptance / refinement blocks per step
    const uint32_t S = 128u / iters;                                              // ladder steps per pick window (iters <= 128)
    const uint32_t thr16 = (uint32_t)((a.thr_logical + 65535u) >> 16);            // logical iff A[31:16] < thr16
    const uint32_t thr_base = lds0 + ev.thr_off;                                  // LDS byte address of this rung's threshold row
    uint32_t nbias = 0u - (thr_base + 16u);
    asm volatile("" : "+s"(nbias));                                               // (one v_add3_u32 per accepted move: n4 + address + nbias)
    uint32_t pk = 0;                                                              // packed descriptor offsets of a pick window
    [[maybe_unused]] uint32_t pa0 = 0, pa1 = 0, pb0 = 0, pb1 = 0;                 // top rung: the window's words A, B
    [[maybe_unused]] uint32_t pf_a = 0, pf_b = 0, pf_c = 0, pf_l = 0;             // the booking wave: log entries fetched ahead, for sample pf_l
    uint32_t ws = (uint32_t)(a.step0 % S);                                        // this step's index within its pick window
    uint64_t wi = a.step0 / S;                                                    // ... and the window's
    auto refresh = [&]() {
        // lane l: the picks of proposals 2l, 2l + 1 of the window (one Philox block), as descriptor offsets
        const u32x4 b = wu_philox(wi * 64u + (uint64_t)lane, kSubWuPick, grp, kWuPickStream + slot, a.seed_lo, a.seed_hi);
        if constexpr (FRAME) {
            // ... and what they do, added to the row of their step (both in one: a step's first proposal is an even one).  A run that starts inside a
            // window builds the rows in front of its first step too.  Only this wave touches the buffer: its LDS operations execute in program order,
            // the fences keep the compiler from moving one lane's stores, atomics and loads across another lane's.
            constexpr uint32_t FS = (uint32_t)wu_frame_steps(WV, CONV, ALPHA, IT);
            wu_lds_rw const frm = (wu_lds_rw)(uintptr_t)(lds0 + ev.frm_off);
#pragma unroll
            for (uint32_t i = 0; i < (FS * FW + 63u) / 64u; ++i) {
                const uint32_t at = i * 64u + (uint32_t)lane;
                if (at < FS * FW) frm[at] = 0u;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if ((uint32_t)lane < FS * (uint32_t)IT / 2u) {
                wu_lds_rw const row = frm + ((uint32_t)lane / ((uint32_t)IT / 2u)) * FW;
                auto desc_word = [&](uint32_t g, int i) { return a.wu_desc[(size_t)g * (CODE == kCodeToric ? 8u : 16u) + (uint32_t)i]; };
                auto lml_word = [&](uint32_t kind, uint32_t pos, int w) { return lml[(kind * (uint32_t)(L + 1) + pos) * (uint32_t)WV + (uint32_t)w]; };
                auto xor_word = [&](uint32_t w, uint32_t v) { __hip_atomic_fetch_xor(row + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
                wu_frame_add<CODE, WV>(b.x, b.y, thr16, G, L, desc_word, lml_word, xor_word);
                wu_frame_add<CODE, WV>(b.z, b.w, thr16, G, L, desc_word, lml_word, xor_word);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        } else {
        const uint32_t g0 = scale_u32(b.y, G), g1 = scale_u32(b.w, G);
        pk = CODE == kCodeToric ? (g0 << 5) | (g1 << 21) : (g0 << 6) | (g1 << 22);
        if (top) { pa0 = b.x; pb0 = b.y; pa1 = b.z; pb1 = b.w; }
        }
    };
    refresh();
    // The waves below the top of the lean kernels with the unrolled loop carry the step's acceptance block (one per step: iters = 10) from the tail of
    // the step before, where it is drawn behind the second barrier: the block is addressed by (T, ladder, slot) and by nothing a step decides, and in
    // the once-per-workgroup form of the cascade these waves have nothing else to issue there while the top rung's wave walks the pairs.  The first
    // step's is drawn here; the last step draws one that nobody reads (a resumed run draws it again in front of its loop).
    constexpr bool AHEAD = LEAN && !TOP && IT == 10;
    [[maybe_unused]] u32x4 abn{0, 0, 0, 0};
    if constexpr (AHEAD) abn = wu_philox(a.step0, kSubWuAcc, syn, slot, a.seed_lo, a.seed_hi);
    // The walk on bounds the waves below the top found (wu_once == 2; the lean tail below has the schedule): in step T the top rung's wave draws the swap
    // words of step T + 1 and stores them raw behind its walk, and the wave of slot s turns row s of swd -- pair s -- into the bound somewhere between that
    // step's third barrier and the next step's first.  The first step of a launch (of every resumed chunk) has no step before it: its words are drawn and
    // stored here, in front of ONE barrier outside the step loop, which every wave of the workgroup meets (wu_once is uniform over the launch).
    constexpr bool SPREAD = LEAN && !STATS && !LONG && wu_frame_steps(WV, CONV, ALPHA, IT) != 0;
    if constexpr (SPREAD) {
        if (a.wu_once == 2u) {
            const int NC = a.Nc;
            const WuLds ol = wu_lds(NC, WV, a.ncls, 0, false, false);
            const uint32_t col = lds0 + (uint32_t)lane * 4u;
            if constexpr (TOP) {
                wu_lds_rw const swd0 = (wu_lds_rw)(uintptr_t)(col + (uint32_t)ol.swd * 4u);
                wu_put_block(swd0, wu_philox(a.step0, 0u, syn, kSwapStream, a.seed_lo, a.seed_hi), NC - 1);
                if (NC > 5) wu_put_block(swd0 + 256, wu_philox(a.step0, 1u, syn, kSwapStream, a.seed_lo, a.seed_hi), NC - 5);
            }
            __syncthreads();
            if constexpr (!TOP && kWuSpreadAt == 0) {
                wu_lds_rw const row = (wu_lds_rw)(uintptr_t)(col + (uint32_t)(ol.swd + (int)slot * 64) * 4u);
                row[0] = wu_bound_word(a, row[0], lds0 + (uint32_t)(ol.swapT + (int)slot * kSwapFast) * 4u, (int)slot);
            }
        }
    }

    // (the criterion kernels book a step behind the barrier of the next one: without the queue one more, unbooked, step follows the last)
    for (uint64_t t = 0; QUEUE || t < a.nsteps + (CONV ? 1u : 0u); ++t) {
        if constexpr (wu_prio_family(WV, ALPHA)) wu_step_priority((uint32_t)t);   // the workgroup's issue priority falls as it advances
        // the ladder's own step: what addresses its acceptance and swap uniforms
        const uint64_t T = QUEUE ? (uint64_t)((uint32_t)t - t0) : a.step0 + t;
        [[maybe_unused]] uint32_t maskv = 0, cdelta = 0;                           // top rung: the step's frame of logical operators (lane w: word w), class change
        const uint32_t pbase = ws * iters;                                         // the step's first proposal within the window
        [[maybe_unused]] WuAl al{0u, 0u, 0u};
        if constexpr (ALPHA && !top) al.Nb = wu_counts_packed<WV>(st, m55, a.W);   // p_b's counts (mcmc_alpha.py:38-41)
        if constexpr (FRAME) {
            // the step's row: lane w < WV takes the mask of word w, the lanes from WV on the class change
            const uint32_t fv = ((wu_lds_ptr)(uintptr_t)(lds0 + ev.frm_off))[ws * FW + (uint32_t)(lane < WV ? lane : WV)];
            maskv = fv;
            cdelta = (uint32_t)__builtin_amdgcn_readlane((int)fv, WV);
        } else
        for (uint32_t c = 0; c < nch; ++c) {
            [[maybe_unused]] u32x4 ab{0, 0, 0, 0};                                 // this ladder's block of ten 12-bit acceptance uniforms
            if constexpr (AHEAD) ab = abn;                                         // (drawn in the tail of the step before)
            else if (!top) ab = wu_philox(T * nch + c, kSubWuAcc, syn, slot, a.seed_lo, a.seed_hi);
            uint32_t left = iters - c * 10u;
            if constexpr (IT == 0) asm volatile("" : "+s"(left));                  // (a scalar bound for the guards below)
#pragma unroll
            for (int f = 0; f < 10; ++f) {
                if constexpr (IT == 0) { if ((uint32_t)f >= left) continue; }     // (skipped, not left: a loop with one exit unrolls)
                const uint32_t P = pbase + c * 10u + (uint32_t)f;                  // proposal of the window: lane P >> 1, half P & 1
                if constexpr (!top && IT == 10) { if (f & 1) continue; }           // (done with its pair)
                // (iters = 10: a step's first proposal sits at an even index of its window, so the lane that holds proposal P is half the step's
                // base plus a constant)
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)pk, IT == 10 ? (int)((pbase >> 1) + ((c * 10u + (uint32_t)f) >> 1)) : (int)(P >> 1));
                const uint32_t off = (P & 1u) ? r >> 16 : r & 0xFFFFu;
                // (byte offsets: multiples of the descriptor's 64 bytes, toric 32 -- added to the table's address as they are)
                typedef const char __attribute__((address_space(4))) *wu_const_bytes;
                const wu_const_ptr e = (wu_const_ptr)((wu_const_bytes)desc + off);
                if constexpr (top) {
                    const uint32_t A = (uint32_t)__builtin_amdgcn_readlane((int)((P & 1u) ? pa1 : pa0), (int)(P >> 1));
                    // a logical operator (mcmc.py:23-24; toric_model.py:228-253, xzzx_model.py:340-357) goes into the frame; a stabilizer is applied
                    // unseen (mcmc.py:30); wu_logical (wu_frames.hpp): the operators that act and what they change of the class
#define QECMC_WU_LOGICAL()                                                                                                       \
                        const uint32_t B = (uint32_t)__builtin_amdgcn_readlane((int)((P & 1u) ? pb1 : pb0), (int)(P >> 1)); \
                        const int LW = (L + 1) * WV; \
                        cdelta ^= wu_logical<CODE>(A, B, L, [&](uint32_t kind, uint32_t pos) { maskv ^= lml[kind * LW + pos * WV + lane]; });
                    if constexpr (WV == 32) {
                        // (32 words: a logical proposal passes through the stabilizer's XOR too, with zeros, so that the state tuple has ONE path
                        // through the loop body -- a branch around an asm statement that updates the tuple makes the compiler merge two copies of it
                        // where the paths meet, which at 32 words is a round trip of the whole state through scratch per step.  The narrower
                        // kernels keep the branch: their merge costs nothing, and the unified form costs the headline kernel 8 B of scratch.)
                        const bool logical = thr16 != 0 && (A >> 16) < thr16;
                        if (logical) { QECMC_WU_LOGICAL() }
                        if constexpr (CODE == kCodeToric) {
                            const wu_desc8 d = *(wu_const_desc8)e;
                            wu_xor_cell<WV>(st, d[0], d[1], d[2], logical ? 0u : d[3], logical ? 0u : d[4], logical ? 0u : d[5]);
                        } else {
                        const uint32_t d0 = e[0], d1 = e[1], d2 = e[2], d3 = e[3];
                        const uint32_t x0 = logical ? 0u : e[4], x1 = logical ? 0u : e[5], x2 = logical ? 0u : e[6], x3 = logical ? 0u : e[7];
                        wu_xor<WV>(st, d0, d1, d2, d3, x0, x1, x2, x3);
                        }
                    } else {
                        if (thr16 != 0 && (A >> 16) < thr16) {
                            QECMC_WU_LOGICAL()
                        } else if constexpr (CODE == kCodeToric) {
                            const wu_desc8 d = *(wu_const_desc8)e;
                            wu_xor_cell<WV>(st, d[0], d[1], d[2], d[3], d[4], d[5]);
                        } else {
                            const uint32_t d0 = e[0], d1 = e[1], d2 = e[2], d3 = e[3], x0 = e[4], x1 = e[5], x2 = e[6], x3 = e[7];
                            wu_xor<WV>(st, d0, d1, d2, d3, x0, x1, x2, x3);
                        }
                    }
#undef QECMC_WU_LOGICAL
                } else {
                    const uint32_t j = c * 10u + (uint32_t)f;
                    if constexpr (IT == 10) {
                        // (iters even: proposal parity = field parity; a lane of the window holds a pair: one readlane, both descriptors
                        // fetched together, the second one's latency hidden behind the first proposal)
                        if constexpr (ALPHA) {
                          if ((f & 1) == 0) {
                            const wu_const_ptr eb = (wu_const_ptr)((wu_const_bytes)desc + (r >> 16));
                            const uint32_t d0 = e[0], d1 = e[1], d2 = e[2], d3 = e[3], x0 = e[4], x1 = e[5], x2 = e[6], x3 = e[7];
                            const uint32_t am = e[11], tlo = e[12], thi = e[13], om = e[14], coff = e[15];
                            const uint32_t b0 = eb[0], b1 = eb[1], b2 = eb[2], b3 = eb[3], y0 = eb[4], y1 = eb[5], y2 = eb[6], y3 = eb[7];
                            const uint32_t an = eb[11], ulo = eb[12], uhi = eb[13], on = eb[14], cofn = eb[15];
                            __builtin_amdgcn_sched_barrier(0);
                            wu_propose_alpha<CODE, WV>(a, st, al, wu_field(ab, f), cht_base + coff, lxyf, lzf, d0, d1, d2, d3, x0, x1, x2, x3, tlo, thi, om, am,
                                                       T * nc4 + (j >> 2), j & 3u, syn, slot, m55);
                            wu_propose_alpha<CODE, WV>(a, st, al, wu_field(ab, f + 1), cht_base + cofn, lxyf, lzf, b0, b1, b2, b3, y0, y1, y2, y3, ulo, uhi, on, an,
                                                       T * nc4 + ((j + 1u) >> 2), (j + 1u) & 3u, syn, slot, m55);
                          }
                        } else if constexpr (CODE == kCodeToric) {
                          if ((f & 1) == 0) {
                            // (seven scalars per proposal, one s_load_dwordx8 each)
                            const wu_desc8 da = *(wu_const_desc8)e, db = *(wu_const_desc8)((wu_const_bytes)desc + (r >> 16));
                            __builtin_amdgcn_sched_barrier(0);
                            wu_propose<CODE, WV>(st, n4, wu_field(ab, f), thr_base, nbias, da[0], 0u, da[1], da[2], da[3], 0u, da[4], da[5], da[6], 0u, 0u, 0u,
                                                 T * nc4 + (j >> 2), j & 3u, syn, slot, a.seed_lo, a.seed_hi);
                            wu_propose<CODE, WV>(st, n4, wu_field(ab, f + 1), thr_base, nbias, db[0], 0u, db[1], db[2], db[3], 0u, db[4], db[5], db[6], 0u, 0u, 0u,
                                                 T * nc4 + ((j + 1u) >> 2), (j + 1u) & 3u, syn, slot, a.seed_lo, a.seed_hi);
                          }
                        } else
                        if ((f & 1) == 0) {
                            const wu_const_ptr eb = (wu_const_ptr)((wu_const_bytes)desc + (r >> 16));
                            const uint32_t d0 = e[0], d1 = e[1], d2 = e[2], d3 = e[3], x0 = e[4], x1 = e[5], x2 = e[6], x3 = e[7], tlo = e[8];
                            const uint32_t thi = e[9], om = e[10], am = e[11];
                            const uint32_t b0 = eb[0], b1 = eb[1], b2 = eb[2], b3 = eb[3], y0 = eb[4], y1 = eb[5], y2 = eb[6], y3 = eb[7], ulo = eb[8];
                            const uint32_t uhi = eb[9], on = eb[10], an = eb[11];
                            __builtin_amdgcn_sched_barrier(0);
                            wu_propose<CODE, WV>(st, n4, wu_field(ab, f), thr_base, nbias, d0, d1, d2, d3, x0, x1, x2, x3, tlo, thi, om, am,
                                                 T * nc4 + (j >> 2), j & 3u, syn, slot, a.seed_lo, a.seed_hi);
                            wu_propose<CODE, WV>(st, n4, wu_field(ab, f + 1), thr_base, nbias, b0, b1, b2, b3, y0, y1, y2, y3, ulo, uhi, on, an,
                                                 T * nc4 + ((j + 1u) >> 2), (j + 1u) & 3u, syn, slot, a.seed_lo, a.seed_hi);
                        }
                    } else if constexpr (ALPHA) {
                        const uint32_t d0 = e[0], d1 = e[1], d2 = e[2], d3 = e[3], x0 = e[4], x1 = e[5], x2 = e[6], x3 = e[7];
                        const uint32_t am = e[11], tlo = e[12], thi = e[13], om = e[14], coff = e[15];
                        wu_propose_alpha<CODE, WV>(a, st, al, wu_field(ab, f), cht_base + coff, lxyf, lzf, d0, d1, d2, d3, x0, x1, x2, x3, tlo, thi, om, am,
                                                   T * nc4 + (j >> 2), j & 3u, syn, slot, m55);
                    } else if constexpr (CODE == kCodeToric) {
                        const wu_desc8 d = *(wu_const_desc8)e;
                        wu_propose<CODE, WV>(st, n4, wu_field(ab, f), thr_base, nbias, d[0], 0u, d[1], d[2], d[3], 0u, d[4], d[5], d[6], 0u, 0u, 0u,
                                             T * nc4 + (j >> 2), j & 3u, syn, slot, a.seed_lo, a.seed_hi);
                    } else {
                        const uint32_t d0 = e[0], d1 = e[1], d2 = e[2], d3 = e[3], x0 = e[4], x1 = e[5], x2 = e[6], x3 = e[7], tlo = e[8];
                        const uint32_t thi = e[9], om = e[10], am = e[11];
                        wu_propose<CODE, WV>(st, n4, wu_field(ab, f), thr_base, nbias, d0, d1, d2, d3, x0, x1, x2, x3, tlo, thi, om, am,
                                             T * nc4 + (j >> 2), j & 3u, syn, slot, a.seed_lo, a.seed_hi);
                    }
                }
            }
        }
        if (top) {
            // the step's logical operators at once, then the error count (the blind moves did not keep it)
            cls ^= cdelta;
            n4 = 0;
            [[maybe_unused]] uint32_t tx = 0, tz = 0, txy = 0;
#define QECMC_WU_FLUSH(w)                                                                                    \
            if constexpr (w < WV) {                                                                          \
                wu_xor_s<WV, w>(st, (uint32_t)__builtin_amdgcn_readlane((int)maskv, w));                     \
                if constexpr (ALPHA) wu_count3<WV, w>(st, tx, tz, txy, m55);                                 \
                else wu_count<WV, w>(st, n4, m55);                                                           \
            }
            WU_EACH(QECMC_WU_FLUSH)
#undef QECMC_WU_FLUSH
            if constexpr (ALPHA) { n4 = tz + txy; nef = tz | (txy << 16); }           // (every move of this rung is accepted: the attribute follows, :58)
            n4 <<= 2;
        } else if constexpr (ALPHA) {
            // the counts the step ends with; the slot's attribute follows them if a move was accepted (mcmc_alpha.py:70)
            const wu_half2 D = __builtin_bit_cast(wu_half2, al.Dh);
            const uint32_t ez = (uint32_t)((int)((al.Nb >> 10) & 1023u) + (int)(float)D.y), exy = (uint32_t)((int)(al.Nb >> 20) + (int)(float)D.x);
            n4 = (ez + exy) << 2;
            if (al.any) nef = ez | (exy << 16);
        }
        // the next step's pick window (state-independent; before the barrier, where the other waves are still busy)
        if (++ws == S) { ws = 0; ++wi; refresh(); }

        if constexpr (LEAN) {
        // ---- Ladder.step's swap sweep (mcmc.py:96-103) of the fixed-length kernels of up to 16 words under the depolarizing rule.  A rung's region of
        // the exchange buffer is WV rows (wu_rows), so everything the tail addresses sits at a multiple of Nc behind one per-lane base: a few
        // scalar instructions per step, formed here from laundered copies of the shape -- hoisted, they would be spilled across the proposal loop.
        int NCl = a.Nc, ncl = a.ncls;
        uint32_t slotl = ev.slot, lds0l = ev.lds0, once = a.wu_once;
        asm volatile("" : "+s"(NCl), "+s"(ncl), "+s"(slotl), "+s"(lds0l), "+s"(once));
        if constexpr (STATS || LONG) once = 0;             // (the replay: every wave decides the pair below its own slot; more than 8 rungs: never walked once)
        const int NC = NCl;
        const uint32_t slot = slotl;
        const WuLds ol = wu_lds(NC, WV, ncl, 0, false, false);                       // (the offsets up to swapT: functions of Nc, WV and ncls alone)
        constexpr uint32_t xstride = (uint32_t)WV * 256u;                            // bytes of one rung in the exchange buffer
        const uint32_t xaddr = lds0l + (uint32_t)lane * 4u;
        wu_lds_rw const recl = (wu_lds_rw)(uintptr_t)(xaddr + (uint32_t)ol.rec * 4u), swdl = recl + NC * 64;   // rec[lane], swd[lane]
        const uint32_t tb0 = lds0l + (uint32_t)ol.swapT * 4u;
        const int swb = NC - 1 - (int)slot;                 // the top rungs draw the swap uniforms: block swb = pairs 4 swb .. 4 swb + 3
        // (the kernels of up to 8 rungs whose top role is the frame role: that role is the lightest of the workgroup by a third, so its wave draws both
        // blocks such a ladder has -- the words are addressed by (T, block, ladder), the same in every wave -- and the waves below it carry neither the
        // test nor the call: -1.7 % at 8 rungs, -2.8 % at 6.  LONG, the 1 024-thread kernels, keep a block per wave: +1.5 % at 12 rungs with the top
        // wave drawing two)
        constexpr bool TOPDRAWS = !LONG && wu_frame_steps(WV, CONV, ALPHA, IT) != 0;
        // Behind the draw, still in front of the first barrier, the drawer turns every word into its pair's bound (wu_bound_block): the rows of swd hold
        // bounds, and the cascade below compares.
        // once == 2 (a TOPDRAWS kernel's walk; STATS and LONG have folded it to 0): the bounds are spread over the waves below the top.  The top wave draws
        // the words of step T + 1 here, keeps them raw in registers up to its walk and stores them behind the walk's reads, into the rows it has just
        // read: in a walked step nobody but the walker reads swd.  The wave of slot s converts row s in place (own_bound) between the step's last
        // barrier and the next step's first, and nobody else touches row s from that last barrier to the walker's read in the next step (behind its first
        // barrier; in a build of three barriers behind its second): the step gets no barrier for it.  The addressing of the words is unchanged -- only who turns a word into a bound, and when.
        const bool spread = once == 2u;
        u32x4 sb{0, 0, 0, 0};
        [[maybe_unused]] u32x4 sb1{0, 0, 0, 0};
        [[maybe_unused]] bool duty = false;
        auto bound_block = [&](int blk, u32x4 &v) { wu_bound_block(a, v, tb0 + (uint32_t)(blk * 4) * (uint32_t)(kSwapFast * 4), blk * 4, NC - 1 - blk * 4); };
        if constexpr (TOPDRAWS && TOP) {
            // (two stretches of straight-line code: the walk on the top wave's own bounds keeps the parent's order of draw and bounds.  One draw site with a
            // selected step number measured the same in both forms, profiles/r15_wave_spread_ab.json)
            if (spread) {
                sb = wu_philox(T + 1u, 0u, syn, kSwapStream, a.seed_lo, a.seed_hi);
                if (NC > 5) sb1 = wu_philox(T + 1u, 1u, syn, kSwapStream, a.seed_lo, a.seed_hi);
            } else {
                sb = wu_philox(T, 0u, syn, kSwapStream, a.seed_lo, a.seed_hi);
                if (NC > 5) sb1 = wu_philox(T, 1u, syn, kSwapStream, a.seed_lo, a.seed_hi);
                bound_block(0, sb);
                if (NC > 5) bound_block(1, sb1);
            }
        } else if constexpr (!TOPDRAWS) {
            duty = swb >= 0 && swb < 4 && swb * 4 < NC - 1;
            if (duty) {
                sb = wu_philox(T, (uint32_t)swb, syn, kSwapStream, a.seed_lo, a.seed_hi);
                bound_block(swb, sb);
            }
        }
        auto put_block = [&](int blk, const u32x4 &v) { wu_put_block(swdl + (uint32_t)(blk * 4) * 64u, v, NC - 1 - blk * 4); };
        // (a wave below the top, once == 2: the word of the pair above its slot, read, turned into the bound and stored in one place -- the role has no
        // register to carry it across the proposal loop)
        [[maybe_unused]] auto own_bound = [&]() {
            wu_lds_rw const row = swdl + slot * 64u;
            row[0] = wu_bound_word(a, row[0], tb0 + slot * (uint32_t)(kSwapFast * 4), (int)slot);
        };
        if constexpr (TOPDRAWS && !TOP && kWuSpreadAt == 1) { if (spread) own_bound(); }
        // this wave's record, and the bounds of the pairs whose words it drew (once == 2: the top wave's words stay raw in registers, above)
        auto publish = [&]() {
            recl[slot * 64u] = pack_info(n4 >> 2, slot, cls, flag);
            if constexpr (TOPDRAWS && TOP) {
                if (!spread) {
                    put_block(0, sb);
                    if (NC > 5) put_block(1, sb1);
                }
            } else if constexpr (!TOPDRAWS) {
                if (duty) put_block(swb, sb);
            }
        };
        // the next step's acceptance block (AHEAD, above): walked once, it fills the wait for the step's last barrier; replayed, the draw has merely moved
        // behind the second barrier from the top of the step.  No barrier and no LDS access inside.
        // (wu_philox launders the seed in front of the block and the statement behind it takes the four words: the draw stays between the two, and
        // these between the barriers -- left alone, the compiler sinks the whole block to the loop's latch, behind the exchange)
        auto draw_ahead = [&]() {
            if constexpr (AHEAD) {
                abn = wu_philox(T + 1u, kSubWuAcc, syn, slot, a.seed_lo, a.seed_hi);
                asm volatile("" : "+v"(abn.x), "+v"(abn.y), "+v"(abn.z), "+v"(abn.w));
            }
        };
        // The cascade once per workgroup: the top rung's wave walks the pairs top-down and leaves in rec[i] the record slot i now holds (rec[i + 1] is dead
        // once pair i is decided: `car` has it); behind the step's last barrier a wave reads its slot's.  Every read the walk needs is issued in front of its
        // first decision -- the records, and beside each the bound of the pair below it, counted from the top: constant offsets from one base, at most 8 rungs
        // here (!LONG) -- and waited for once; the chain itself runs in registers, a compare and two selects per pair on ne(lo) + D, which is formed off the
        // chain.  The stores of rec[i + 1] go out as the chain advances and are waited for in front of the barrier alone.  Returns rung 0's new record.
        // At fewer than 8 rungs (the walk serves 5 .. 8) the record loads of "slots below 0" (r[NC] .. r[7]) fall into the last 8 - NC rows of the exchange
        // buffer, which lies in front of rec -- rows of the top rung's own region, which in the two-barrier step the walker itself stores into behind these
        // loads, while the other waves store into theirs -- and the bound loads of "pairs below 0" (s[NC - 1] .. s[6]) into rows 2 NC - 8 .. NC - 1 of rec.
        // No such value reaches a use: the chain reads r[0], r[j + 1] and s[j] for j < NC - 1 alone, and the sums s[j] += r[j + 1] of j >= NC - 1 end in
        // registers nobody reads.
        // Two halves -- the loads, then the wait and the chain --, because the two-barrier step issues the walker's own state stores between them, in the
        // wait for the loads, and those stand on the path every form shares: a state store (an asm statement that names the pinned tuple) inside a branch
        // makes the compiler merge two copies of the tuple where the paths meet, a round trip of the state through scratch per step.
        [[maybe_unused]] uint32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s[7] = {0, 0, 0, 0, 0, 0, 0};
        [[maybe_unused]] auto walk_loads = [&]() __attribute__((always_inline)) {
            wu_lds_ptr const pr = recl + (NC - 8) * 64, px = swdl + (NC - 8) * 64;
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = pr[64 * (7 - j)];                  // slot NC - 1 - j's record
#pragma unroll
            for (int j = 0; j < 7; ++j) s[j] = px[64 * (6 - j)];                  // pair NC - 2 - j's bound
        };
        [[maybe_unused]] auto walk_chain = [&]() __attribute__((always_inline)) {
            wu_lds_rw const pr = recl + (NC - 8) * 64;
            asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]),
                              "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]), "+v"(s[4]), "+v"(s[5]), "+v"(s[6]));   // (all of them here: one wait)
            if constexpr (TOPDRAWS) {
                // (the next step's raw words, into the rows just read: the stores go out beside the chain and are waited for in front of the barrier)
                if (spread) {
                    put_block(0, sb);
                    if (NC > 5) put_block(1, sb1);
                }
            }
#pragma unroll
            for (int j = 0; j < 7; ++j) s[j] += r[j + 1] & 0xFFFFu;
            uint32_t car = r[0], nc = car & 0xFFFFu;
#pragma unroll
            for (int j = 0; j < 7; ++j) {                                        // pair i = NC - 2 - j, mcmc.py:96
                if (j < NC - 1) {
                    const uint32_t lo = r[j + 1];
                    const bool flip = nc <= s[j];                                // ne_hi - ne_lo <= D
                    pr[64 * (7 - j)] = flip ? lo : car;                             // what slot i + 1 now holds (:98-99)
                    car = flip ? car : lo;
                    nc = flip ? nc : lo & 0xFFFFu;
                }
            }
            recl[0] = car;
            return car;
        };
        // ladder + PTEQ bookkeeping on rung 0's new record: by the wave of slot 0, or -- a build with kWuTopBooks, walked -- by the walker, which ends its
        // chain holding that record (`car`, what it stored to rec[0]).  Whoever books carries tops0 and samples, and is the only wave that touches hist
        // (ladder_wu_body.inc loads a resumed run's tops0 into that wave and hands both values to wave 0's write-out behind the loop).
        auto book = [&](uint32_t fl, uint32_t c0) {                                  // r0's flag and class
            tops0 += (NC == 1) | fl;                                                 // :101-102
            if (a.counts != nullptr && tops0 >= a.tops_burn) {                       // decoders.py:60-67
                wu_lds_rw const hist = (wu_lds_rw)(uintptr_t)(xaddr + (uint32_t)ol.hist * 4u);
                hist[(CODE == kCodeXzzx ? (c0 ^ (c0 >> 1)) : c0) * 64] += 1;
                samples++;
            }
        };
        constexpr bool TBOOKS = wu_top_books_family(WV, CONV, ALPHA, STATS, LONG);
        constexpr bool WALKS = !STATS && !LONG;            // (the kernels in which `once` can be non-zero)
        // The walked forms' step of TWO barriers (kWuStepBarriers == 2), B1 and B3 -- the replay below keeps B1, B2.  Who touches what, per lane column:
        //   exchange buffer, region of rung s: wave s stores it between B1 and B3 (wu_put_all; the walker behind its loads); any wave may take it, between B3
        //             and the next step's B1 (wu_take_all waits for its data).  B1: every take of step T - 1 is done before a row is overwritten; B3: every
        //             store is complete -- each wave waits for its own (wu_ds_drain) in front of it -- before a row is taken.
        //   rec[s]:   wave s publishes it in FRONT of B1 -- behind its own read of the row, `mine`, in program order --; the walker reads it and rewrites it in
        //             place between B1 and B3; wave s reads it behind B3.  Every cross-wave access is the walker's and lies between the two barriers; no third
        //             wave ever addresses row s (a wave's only rec address is its slot's row).
        //   swd[i]:   once == 1, and the kernels whose lower waves draw (no TOPDRAWS): whoever drew the block stores the bounds in front of B1, the walker
        //             reads them between B1 and B3, its reads of step T - 1 lie in front of that step's B3.  once == 2: the walker stores the raw word of step
        //             T + 1 behind its reads, in front of B3; wave i turns it into the bound in place between B3 and the next step's B1 (own_bound); the
        //             walker reads behind that B1 -- the hand-over of the three-barrier step with B1 in B2's place.  Nobody but the walker and wave i
        //             addresses row i.  "The conversion's store is complete at B1": the barrier's own wait covers it, as it covers the record's.
        // So B1 now means "everybody has taken, every record is published, every bound is stored", and the walker starts right behind it.
        const bool two = WALKS && kWuStepBarriers == 2 && once != 0;
        if (two) publish();
        __syncthreads();                                   // B1 (everybody has read the exchange buffer, the records and the swap uniforms of the step before)
        uint32_t mine;
        [[maybe_unused]] uint32_t car0 = 0;                 // the walker: rung 0's new record
        if constexpr (TOP && WALKS && !kWuWalkPutsFirst) { if (two) walk_loads(); }
        wu_put_all<WV>(st, xaddr + slot * xstride);        // (every form, on the one path: the walker's go out in the wait for its loads)
        if (two) {
            if constexpr (TOP && WALKS) {
                if constexpr (kWuWalkPutsFirst) walk_loads();
                car0 = walk_chain();
            }
            draw_ahead();                                  // (the waves below the top: in the walk's shadow, behind their stores)
            wu_ds_drain();                                 // (the asm stores of the exchange are not in the compiler's count)
            __syncthreads();                               // B3
            mine = recl[slot * 64u];
            if constexpr (TBOOKS && TOP) book(car0 >> 31, (car0 >> 24) & 0x3Fu);     // (here, under the form's own test: no test of its own)
        } else {
        publish();
        // (the asm stores of the exchange are not in the compiler's count; the kernels without the fork above keep the statement that names the tuple)
        if constexpr (WALKS && kWuStepBarriers == 2) wu_ds_drain(); else wu_ds_wait<WV>(st);
        __syncthreads();                                   // B2
        draw_ahead();                                      // (one call site for the replay and the three-barrier walk)
        if (kWuStepBarriers != 2 && once) {
            // the three-barrier walk: stores and records behind B1, B2, the walk, B3
            if constexpr (TOP && WALKS) { walk_loads(); car0 = walk_chain(); }
            __syncthreads();
            mine = recl[slot * 64u];
            if constexpr (TBOOKS && TOP) book(car0 >> 31, (car0 >> 24) & 0x3Fu);
        } else {
            // every wave replays the top-down cascade on the published records: the pairs above its slot move `car` alone, the pair below it decides
            wu_lds_ptr pr = recl + (NC - 2) * 64, px = swdl + (NC - 2) * 64;
            uint32_t car = pr[64];
            for (int i = NC - 2; i >= (int)slot; --i) {                              // mcmc.py:96
                const uint32_t lo = pr[0];
                car = wu_bound_flips(car, lo, px[0]) ? car : lo;
                pr -= 64; px -= 64;
            }
            mine = car;
            if (slot != 0) {
                const uint32_t lo = pr[0];
                if (wu_bound_flips(car, lo, px[0])) {
                    mine = lo;                                                          // what slot i + 1 now holds (:98-99)
                    if constexpr (STATS) swapc += 1u;
                }
            }
        }
        }
        wu_take_all<WV>(st, xaddr + ((mine >> 16) & 0xFFu) * xstride);               // this rung's new state: the words of the rung it comes from
        if constexpr (TOPDRAWS && !TOP && kWuSpreadAt == 0) { if (spread) own_bound(); }   // (the next step's bound of this wave's pair: the first step's, in front of the loop)
        n4 = (mine & 0xFFFFu) << 2; cls = (mine >> 24) & 0x3Fu; flag = mine >> 31;
        if constexpr (STATS) nsum += mine & 0xFFFFu;
        if (top) flag = 1;                                                           // chains[-1].flag = 1, mcmc.py:100
        if (slot == 0) {
            if (!(TBOOKS && once)) book(flag, cls);
            flag = 0;                                                                // :103
        }
        } else {
        // ---- Ladder.step's swap sweep (mcmc.py:96-103)
        // (per-step work: its table addresses are formed here, from laundered copies of the shape, instead of being hoisted out of the
        // step loop and kept -- spilled -- in scalar registers across the proposal loop, which runs at 8 waves per SIMD on ~80 SGPRs)
        int NCl = a.Nc, nql = a.nq, ncl = a.ncls, Ll = a.L, Wl = a.W;
        uint32_t slotl = ev.slot, lds0l = ev.lds0;
        asm volatile("" : "+s"(NCl), "+s"(nql), "+s"(ncl), "+s"(Ll), "+s"(slotl), "+s"(lds0l), "+s"(Wl));
        const int NC = NCl, nq = nql, ncls = ncl;
        const uint32_t slot = slotl;
        const WuLds ol = wu_lds(NC, Wl, ncls, Ll, CONV, ALPHA, SHORT);
        // (LDS pointers by address space: a laundered generic pointer would turn every access below into a flat load)
        wu_lds_rw const ldsl = (wu_lds_rw)(uintptr_t)lds0l;
        wu_lds_rw const rec = ldsl + ol.rec, swd = ldsl + ol.swd, hist = ldsl + ol.hist, swapT = ldsl + ol.swapT;
        volatile __attribute__((address_space(3))) uint32_t *const stopf = ldsl + ol.stop;
        [[maybe_unused]] wu_lds_rw const bk = ldsl + ol.bk + (uint32_t)lane, mail = ldsl + ol.mail, bot = ldsl + ol.bot, bot2 = ldsl + ol.bot2;
        [[maybe_unused]] wu_lds_drw const nefd = (wu_lds_drw)(ldsl + ol.nef) + (uint32_t)lane;
        [[maybe_unused]] wu_lds_dptr const lnbd = (wu_lds_dptr)(ldsl + ol.lnb);
        [[maybe_unused]] wu_lds_rw const skey = ldsl + ol.skey + (uint32_t)lane, sst = ldsl + ol.sst + (uint32_t)lane;   // SHORT: [2][2][64] keys, [kShortRows][64] state
        const uint32_t xaddr = lds0l + (uint32_t)lane * 4u;
        constexpr bool PAD = WV == 32 || !CONV;                                      // (wu_rows: padded rows, transfers without width tests)
        const uint32_t xstride = (uint32_t)(WV == 32 ? kWuHalf : PAD ? WV : Wl) * 256u;  // bytes of one rung in the exchange buffer
        const int swb = NC - 1 - (int)slot;                 // the top rungs draw the swap uniforms: block swb = pairs 4 swb .. 4 swb + 3
        u32x4 sb{0, 0, 0, 0};
        const bool duty = swb >= 0 && swb < 4 && swb * 4 < NC - 1;
        if (duty) sb = wu_philox(T, (uint32_t)swb, syn, kSwapStream, a.seed_lo, a.seed_hi);
        __syncthreads();                                   // (everybody has read the exchange buffer and the swap uniforms of the step before)
        {
            const uint32_t xo = xaddr + slot * xstride;
            // (a 32-word state passes through the buffer in two halves: words 0-15 here, the rest behind two more barriers below)
#define QECMC_WU_PUT(w) if constexpr (w < WV && w < kWuHalf) { if (WV == 32 || !CONV || w < wu_words_min(WV) || w < Wl) wu_ds_write<WV, w>(st, xo); }
#define QECMC_WU_PUT_HI(w) if constexpr (w < WV && w >= kWuHalf) wu_ds_write<WV, w, w - kWuHalf>(st, xo);
            WU_EACH(QECMC_WU_PUT)
            rec[slot * 64u + (uint32_t)lane] = pack_info(n4 >> 2, slot, cls, flag);
            if constexpr (ALPHA) nefd[slot * 64u] = alpha_neff(nef, a.alpha);
            if (duty) {
                wu_lds_rw p = swd + (uint32_t)(swb * 4) * 64u + (uint32_t)lane;
                const int left = NC - 1 - swb * 4;
                p[0] = sb.x;
                if (left > 1) p[64] = sb.y;
                if (left > 2) p[128] = sb.z;
                if (left > 3) p[192] = sb.w;
            }
        }
        wu_ds_wait<WV>(st);                                 // (the asm stores of the exchange are not in the compiler's count)
        __syncthreads();
        if constexpr (CONV) { if (stopf[t & 1]) break; }    // (written by wave 0 during the step before: uniform for the workgroup)
        {
            // every wave replays the top-down cascade on the published records down to the rung that fills its own slot
            wu_lds_ptr cur = rec + (uint32_t)lane, sx = swd + (uint32_t)lane;
            uint32_t car = cur[(NC - 1) * 64], mine = car;
            const int i_stop = slot == 0 ? 0 : (int)slot - 1;
            for (int i = NC - 2; i >= i_stop; --i) {                                 // mcmc.py:96
                const uint32_t lo = cur[i * 64], x = sx[i * 64];
                bool flip;
                if constexpr (ALPHA) {
                    flip = wu_alpha_flip(x, nefd[(i + 1) * 64], nefd[i * 64], lnbd[i]);   // the slots' attributes: they stay where they are (Q4)
                } else {
                const int d = (int)(car & 0xFFFFu) - (int)(lo & 0xFFFFu);            // ne_hi - ne_lo, _r_flip :146-149
                // x < ceil(p_diff[i]^d 2^32): the LDS table for d < 64 (entry 0 never passes: d <= 0 flips anyway), else the plan's
                const int dd = d < 1 ? 1 : d;
                bool lt = x < swapT[i * kSwapFast + (dd < kSwapFast ? dd : 0)];
                if (dd >= kSwapFast) lt = (uint64_t)x < a.swap_thr[(size_t)i * (nq + 1) + dd];
                flip = d <= 0 || lt;
                }
                const uint32_t into = flip ? lo : car;                               // what slot i+1 now holds (:98-99)
                car = flip ? car : lo;
                if ((int)slot == i + 1) {
                    mine = into;
                    if constexpr (STATS) swapc += flip ? 1u : 0u;
                }
            }
            if (slot == 0) mine = car;
            // this rung's new state: the W words of the rung it comes from
            const uint32_t xin = xaddr + info_sid(mine) * xstride;
#define QECMC_WU_TAKE(w) if constexpr (w < WV && w < kWuHalf) { if (WV == 32 || !CONV || w < wu_words_min(WV) || w < Wl) wu_ds_read<WV, w>(st, xin); }
#define QECMC_WU_TAKE_HI(w) if constexpr (w < WV && w >= kWuHalf) wu_ds_read<WV, w, w - kWuHalf>(st, xin);
            WU_EACH(QECMC_WU_TAKE)
            wu_ds_wait<WV>(st);
            if constexpr (WV == 32) {
                static_assert(WV != 32 || (!CONV && !QUEUE), "the 32-word kernels: fixed-length runs");
                const uint32_t xo = xaddr + slot * xstride;
                __syncthreads();                               // (every wave has taken the lower half of its new state)
                WU_EACH(QECMC_WU_PUT_HI)
                wu_ds_wait<WV>(st);
                __syncthreads();
                WU_EACH(QECMC_WU_TAKE_HI)
                wu_ds_wait<WV>(st);
            }
            n4 = info_n(mine) << 2; cls = info_cls(mine); flag = info_flag(mine);
            if constexpr (STATS) nsum += info_n(mine);
            if (top) flag = 1;                                                       // chains[-1].flag = 1, mcmc.py:100
            if constexpr (!CONV) {
                if (slot == 0) {                                                     // ladder + PTEQ bookkeeping on rung 0's new state
                    tops0 += (NC == 1) | flag;                                       // :101-102
                    if (a.counts != nullptr && tops0 >= a.tops_burn) {               // decoders.py:60-67
                        hist[(CODE == kCodeXzzx ? (cls ^ (cls >> 1)) : cls) * 64 + lane] += 1;
                        samples++;
                    }
                }
            } else if (slot == 0) {
                bot[((uint32_t)t & 1u) * 64u + (uint32_t)lane] = mine;              // (booked by the top rung's wave behind the next step's barrier)
                if constexpr (ALPHA) bot2[((uint32_t)t & 1u) * 64u + (uint32_t)lane] = nef;   // chains[0].n_eff, decoders_biasednoise.py:204
                if constexpr (SHORT) {
                    // the key of (rung 0's new configuration, slot 0's attribute): the padding words are zero in every state, they travel with the rest
                    uint64_t h = kShortKeySeed;
#define QECMC_WU_KEY(w) if constexpr (w < WV) h = short_key_word(h, wu_get<WV, w>(st));
                    WU_EACH(QECMC_WU_KEY)
#undef QECMC_WU_KEY
                    h = short_key_finish(h, alpha_neff(nef, a.alpha));
                    skey[((uint32_t)t & 1u) * 128u] = (uint32_t)h;
                    skey[((uint32_t)t & 1u) * 128u + 64u] = (uint32_t)(h >> 32);
                }
            }
            if constexpr (CONV && TOP) {
                // ---- ladder + PTEQ bookkeeping with the error_based criterion (decoders.py:60-82,93-105), by the wave of the TOP rung
                // and one step behind: rung 0's wave leaves the record that landed in rung 0 at step tb in LDS
                // (by step parity), and this wave books it behind the barrier of step tb + 1, off the critical path of the workgroup.  The
                // per-ladder state lives in LDS between steps.
                auto book = [&](uint64_t tb, uint64_t Tb) {
                    const uint32_t recw = bot[((uint32_t)tb & 1u) * 64u + (uint32_t)lane];
            // the same with the error_based criterion (decoders.py:74-82,93-105); the per-ladder state lives in LDS between steps
            uint32_t b_tops0 = bk[0], b_samples = bk[64], b_burn = bk[128], b_cstart = bk[192], b_cstreak = bk[256], b_state = bk[576];
            uint64_t sumA = (uint64_t)bk[320] | ((uint64_t)bk[384] << 32), sumB = (uint64_t)bk[448] | ((uint64_t)bk[512] << 32);
            [[maybe_unused]] uint64_t sumAxy = 0, sumBxy = 0;
            if constexpr (ALPHA) { sumAxy = (uint64_t)bk[832] | ((uint64_t)bk[896] << 32); sumBxy = (uint64_t)bk[960] | ((uint64_t)bk[1024] << 32); }
            uint32_t has = (b_state >> 3) & 1u, pending = (b_state >> 1) & 3u, done = b_state & 1u;
            const uint32_t Town = (uint32_t)Tb;                                  // the ladder's own step (of the step being booked)
            bool ended = false;
            uint32_t conv_ok = 0;
            if (has && !done && !pending) {
                b_tops0 += (NC == 1) | info_flag(recw);                                  // :101-102
                const uint32_t n0 = info_n(recw), cls0 = info_cls(recw);
                if (a.counts != nullptr && b_tops0 >= a.tops_burn) {             // decoders.py:60-67
                    hist[(CODE == kCodeXzzx ? (cls0 ^ (cls0 >> 1)) : cls0) * 64 + lane] += 1;
                    b_samples++;
                    if constexpr (SHORT) {
                        // decoders_biasednoise.py:128-144 on chains[0].n_eff and the bottom configuration's key (the lane's ladder: bk row 12)
                        const uint32_t kp = ((uint32_t)tb & 1u) * 128u;
                        short_book(a, (uint64_t)bk[768], sst, 64, CODE == kCodeXzzx ? (cls0 ^ (cls0 >> 1)) : cls0,
                                   alpha_neff(bot2[((uint32_t)tb & 1u) * 64u + (uint32_t)lane], a.alpha), (uint64_t)skey[kp] | ((uint64_t)skey[kp + 64u] << 32));
                    }
                    if (!SHORT || a.conv_mode != 0) {
                    // nbr_errors_bottom_chain[since_burn] = count_errors (:68), logged in HBM: series index i in row burn + i of the
                    // lane's column (QUEUE: a column per lane of the grid, rows = the ladder's own steps)
                    const size_t lN = QUEUE ? (size_t)gridDim.x * 64u : (size_t)a.N;
                    // (ALPHA: chains[0].n_eff -- slot 0's attribute, decoders_biasednoise.py:204 -- logged as its two counts, 4 B)
                    typedef typename std::conditional<ALPHA, uint32_t, uint16_t>::type log_t;
                    log_t *mylog = reinterpret_cast<log_t *>(a.nlog) + ((size_t)blockIdx.x * 64u + (size_t)lane);
                    const uint32_t v0 = ALPHA ? bot2[((uint32_t)tb & 1u) * 64u + (uint32_t)lane] : n0;
                    mylog[(size_t)Town * lN] = (log_t)v0;
                    const uint32_t l = b_samples;
                    const auto [a0, b0, c0, a1, b1, c1] = quartile_rows(l);
                    // the (up to three) entries that leave / enter the windows Q2 = series[l/4 : l/2], Q4 = series[3l/4 : l]: old rows of the
                    // log, i.e. HBM round trips -- fetched one sample ahead (below), so that they travel during the proposals of a step
                    // instead of standing on this wave's path (samples below 8 read them in place: their rows are only just written)
                    const bool ahead = pf_l == l && l >= 8u;
                    uint32_t vc = pf_c, vb = pf_b, va = pf_a;
                    if (!ahead) {
                        vc = c1 != c0 ? mylog[(size_t)(b_burn + c0) * lN] : 0u;
                        vb = b1 != b0 ? mylog[(size_t)(b_burn + b0) * lN] : 0u;
                        va = a1 != a0 ? mylog[(size_t)(b_burn + a0) * lN] : 0u;
                    }
                    window_update<ALPHA>(v0, vc, vb, va, sumA, sumB, sumAxy, sumBxy);
                    {   // ... and the next sample's (the burn-in is over: its offset stays)
                        const uint32_t l2 = l + 1u;
                        const uint32_t a2 = l2 >> 2, b2 = l2 >> 1, c2 = (3u * l2) >> 2;
                        pf_c = c2 != c1 ? mylog[(size_t)(b_burn + c1) * lN] : 0u;
                        pf_b = b2 != b1 ? mylog[(size_t)(b_burn + b1) * lN] : 0u;
                        pf_a = a2 != a1 ? mylog[(size_t)(b_burn + a1) * lN] : 0u;
                        pf_l = l2;
                    }
                    }
                } else {
                    b_burn++;                                                    // resulting_burn_in, :71
                }
                if ((!SHORT || a.conv_mode != 0) && b_tops0 >= a.TOPS) {        // :74 (SHORT, conv_mode NONE: the run goes to the horizon)
                    const bool accept = criterion_accepts<ALPHA>(b_samples, sumA, sumAxy, sumB, sumBxy, a.alpha, a.eps);
                    if (accept) {                                                // (pteq_book.hpp's streak_ends, in place: the call changes resource rows)
                        if (b_cstreak >= a.SEQ) { ended = true; conv_ok = 1; }   // :77-78
                        else b_cstreak = b_tops0 - b_cstart;                     // :79
                    } else {
                        b_cstreak = 0;                                           // :81-82
                        b_cstart = b_tops0;
                    }
                }
                if (QUEUE && !ended && (uint64_t)Town + 1u >= a.nsteps) ended = true;   // the horizon: `steps` of the ladder's own steps
            }
            if constexpr (QUEUE) {
                if (pending) pending -= 1;                                       // (a lane between two ladders: the steps it idles are not booked)
                uint32_t give = kWuKeep;
                const uint64_t em = __ballot(ended);
                if (ended) {    // (pteq_book.hpp's store_class_column / store_ladder_results, in place: the calls change resource rows)
                    // ---- a ladder that ended writes its results at once; its lane takes the workgroup's next one -- in lane order
                    // among the lanes that end at the same step, so the assignment does not depend on timing
                    const uint64_t row = (uint64_t)bk[768] / a.replicas;
                    for (int cc = 0; cc < ncls; ++cc) {
                        const uint32_t v = hist[cc * 64 + lane];
                        hist[cc * 64 + lane] = 0;
                        if (a.replicas > 1) { if (v) atomicAdd(a.counts + row * ncls + cc, v); }
                        else a.counts[row * ncls + cc] = v;
                    }
                    const uint32_t sd = Town + 1u;
                    if (a.replicas > 1) {
                        atomicAdd(a.samples + row, b_samples);
                        if (a.tops0 != nullptr) atomicAdd(a.tops0 + row, b_tops0);
                        if (a.steps_done != nullptr) atomicMax(a.steps_done + row, sd);
                        if (a.converged != nullptr && !conv_ok) a.converged[row] = 0;
                    } else {
                        a.samples[row] = b_samples;
                        if (a.tops0 != nullptr) a.tops0[row] = b_tops0;
                        if (a.steps_done != nullptr) a.steps_done[row] = sd;
                        if (a.converged != nullptr) a.converged[row] = (uint8_t)conv_ok;
                    }
                    if constexpr (SHORT) short_store(a, row, sst, 64);            // (one ladder per lane: nothing to reset)
                    b_tops0 = b_samples = b_burn = b_cstart = b_cstreak = 0; sumA = sumB = 0; sumAxy = sumBxy = 0;
                    const uint32_t cand = (uint32_t)stopf[2] + (uint32_t)__popcll(em & ((1ull << lane) - 1ull));
                    give = (uint64_t)cand < ev.chunk_hi ? cand : kWuDead;
                    if (give == kWuDead) has = 0; else { pending = 2; bk[768] = give; }
                }
                // this step's orders: read by every wave behind the NEXT step's barrier (mailbox and flag by step parity)
                mail[((uint32_t)tb & 1u) * 64u + (uint32_t)lane] = give;
                if (lane == 0) { stopf[2] = (uint32_t)stopf[2] + (uint32_t)__popcll(em); }
                if (__all(!has)) stopf[(tb + 2) & 1] = 1;
            } else {
                if (ended) { done = 1; bk[640] = Town + 1u; bk[704] = conv_ok; }   // steps_done, converged
                if (__all(done || !has)) stopf[(tb + 2) & 1] = 1;
            }
            bk[0] = b_tops0; bk[64] = b_samples; bk[128] = b_burn; bk[192] = b_cstart; bk[256] = b_cstreak;
            bk[320] = (uint32_t)sumA; bk[384] = (uint32_t)(sumA >> 32); bk[448] = (uint32_t)sumB; bk[512] = (uint32_t)(sumB >> 32);
            bk[576] = done | (pending << 1) | (has << 3);
            if constexpr (ALPHA) { bk[832] = (uint32_t)sumAxy; bk[896] = (uint32_t)(sumAxy >> 32); bk[960] = (uint32_t)sumBxy; bk[1024] = (uint32_t)(sumBxy >> 32); }
                };
                if (t > 0) book(t - 1, QUEUE ? (uint64_t)((uint32_t)(t - 1) - t0) : a.step0 + t - 1);
            }

            if (slot == 0) flag = 0;                                                 // :103
        }
        if constexpr (QUEUE) {
            // ---- refill: the orders wave 0 wrote during the step before take effect here, behind this step's barrier: every wave stages
            // its own rung of the lane's new ladder (the lane idled this step; its ladder's first step is the next one)
            if (t > 1) {
                const uint32_t give = mail[((uint32_t)t & 1u) * 64u + (uint32_t)lane];          // (the orders of the booking of step t - 2)
                if (__builtin_amdgcn_uicmp(give, kWuKeep, 36) != 0) {                // (some lane has an order: give < kWuKeep -- ICMP_ULT)
                    if (give < kWuKeep) {
                        // (through the lane's own column of this rung's rows of the exchange buffer: whoever still reads that column reads it
                        // for the same lane, whose state is being replaced in every wave)
                        syn = a.first_syndrome + give;
                        t0 = (uint32_t)t + 1u;
                        wu_stage_lds<CODE>(a, (uint64_t)give, slot, ldsl + (slot * (uint32_t)Wl) * 64u + (uint32_t)lane, n4, cls);
                        const uint32_t xme = xaddr + slot * xstride;
#define QECMC_WU_MINE(w) if constexpr (w < WV) { if (w < wu_words_min(WV) || w < Wl) wu_ds_read<WV, w>(st, xme); }
                        WU_EACH(QECMC_WU_MINE)
#undef QECMC_WU_MINE
                        wu_ds_wait<WV>(st);
                        flag = top ? 1u : 0u;
                        if constexpr (ALPHA) { const uint32_t c3 = wu_counts_packed<WV>(st, m55); nef = ((c3 >> 10) & 1023u) | ((c3 >> 20) << 16); }   // Chain_alpha.__init__
                    }
                }
            }
        }
        }
    }
    cx.n4 = n4; cx.cls = cls; cx.flag = flag; cx.tops0 = tops0; cx.samples = samples;
    if constexpr (ALPHA) cx.nef = nef;
    if constexpr (STATS) { cx.swapc = swapc; cx.nsum = nsum; }
}

template <int MAXT, int MINW, int CODE, int WV, bool CONV, bool QUEUE, int IT, bool ALPHA = false>
__global__ __launch_bounds__(MAXT, MINW) void ladder_wu_kernel(const LadderArgs a)
{
    constexpr bool STATS = false, SHORT = false, LONG = MAXT > 512;
#include "ladder_wu_body.inc"
}

// The same program with the swap and per-rung error counters of qecmc_plan_set_stats: a diagnostic kernel of its own name (choose_wave's
// wave_stats_key), fixed-length runs, the general proposal loop, 128 VGPRs under a launch bound of 1 024 threads whatever the ladder's length
template <int CODE, int WV, bool ALPHA>
__global__ __launch_bounds__(1024, 4) void ladder_wu_stats_kernel(const LadderArgs a)
{
    constexpr bool STATS = true, CONV = false, QUEUE = false, SHORT = false, LONG = true;
    constexpr int IT = 0;
#include "ladder_wu_body.inc"
}
// The alpha rule's queue kernel with the shortest-chain statistics of qecmc_plan_set_shortest (choose_shortest's wave_short_key): launched with one ladder
// per lane (a.wu_chunk = 64 on ceil(N / 64) workgroups), so a ladder's results depend on (seed, global ladder index) alone; 1 024 threads at 4 waves per
// SIMD whatever the ladder's length; IT = 10 / 0 as in ladder_wu_kernel
template <int CODE, int WV, int IT>
__global__ __launch_bounds__(1024, 4) void ladder_wu_shortest_kernel(const LadderArgs a)
{
    constexpr bool STATS = false, CONV = true, QUEUE = true, ALPHA = true, SHORT = true, LONG = true;
#include "ladder_wu_body.inc"
}
// (the transfer macros of wu_run's general tail, which the kernels' epilogue shares)
#undef QECMC_WU_PUT
#undef QECMC_WU_TAKE
#undef QECMC_WU_PUT_HI
#undef QECMC_WU_TAKE_HI
template <int CODE, int WV, bool ALPHA = false>
struct WaveStatsSet {
    static const void *find(const KernelKey &k)
    {
        return k == wave_stats_key(CODE, WV, ALPHA) ? (const void *)ladder_wu_stats_kernel<CODE, WV, ALPHA> : nullptr;
    }
};

template <int CODE, int WV>
struct WaveShortestSet {
    static const void *find(const KernelKey &k)
    {
        if (!(k == wave_short_key(CODE, WV, k.it))) return nullptr;
        return k.it == 10 ? (const void *)ladder_wu_shortest_kernel<CODE, WV, 10> : k.it == 0 ? (const void *)ladder_wu_shortest_kernel<CODE, WV, 0> : nullptr;
    }
};

// the instantiations ladder_wu_kernel<MAXT, MINW, CODE, WV, CONV, QUEUE = CONV, IT, ALPHA> for IT = 10 (the unrolled proposal loop of iters = 10)
// and IT = 0 (any iters): find() is the kernel of `k` if it is one of them, else nullptr
template <int MAXT, int MINW, int CODE, int WV, bool CONV, bool ALPHA = false>
struct WaveSet {
    static const void *find(const KernelKey &k)
    {
        if (!(k == wave_key(MAXT, MINW, CODE, WV, CONV, k.it, ALPHA))) return nullptr;
        return k.it == 10 ? (const void *)ladder_wu_kernel<MAXT, MINW, CODE, WV, CONV, CONV, 10, ALPHA>
             : k.it == 0  ? (const void *)ladder_wu_kernel<MAXT, MINW, CODE, WV, CONV, CONV, 0, ALPHA> : nullptr;
    }
};
// a code's kernels of 4 .. 16 state words per rung on MAXT threads (choose_wave, kernel_choice.hpp): fixed-length and criterion runs
template <int MAXT, int CODE>
using WaveWords = KernelList<WaveSet<MAXT, 8, CODE, 4, false>, WaveSet<MAXT, 8, CODE, 8, false>, WaveSet<MAXT, 8, CODE, 12, false>, WaveSet<MAXT, 6, CODE, 16, false>,
                             WaveSet<MAXT, 8, CODE, 4, true>, WaveSet<MAXT, 8, CODE, 8, true>, WaveSet<MAXT, 8, CODE, 12, true>, WaveSet<MAXT, 6, CODE, 16, true>>;

}  // namespace qecmc
