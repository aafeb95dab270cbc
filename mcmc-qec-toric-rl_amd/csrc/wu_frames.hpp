// scan = 3 (ladder_wu.hpp), the top rung's moves as FRAMES.  The top rung accepts every move (mcmc.py:30) and its picks are shared by the 64 ladders of
// a wavefront, so what its `iters` moves of a ladder step do to a state is one wave-uniform XOR mask of the state's words plus a change of the class: a
// row of WV + 1 words.  The rows of a pick window are built when the window is drawn -- lane l holds the picks of proposals 2l, 2l + 1 and adds what they
// do to the row of their step -- and a step of the top rung's wave is then one row read and the flush of the mask.  Host and device share the two
// functions below (tests/test_wave_frames_cpu.py builds a window's rows through tables_test_api.cpp and holds them against the oracle's stencils).
#pragma once
#include <stdint.h>

#include "kernel_choice.hpp"

namespace qecmc {

// The logical operators of a top-rung proposal with pick words A, B (_apply_random_logical: toric_model.py:228-253, xzzx_model.py:340-357; the fields
// of A and B: philox.hpp, the packed layout): row(kind, pos) is called for every operator that acts -- row `pos` of kind `kind` of the logical masks
// [4][L + 1][.] (tables.hpp) --, the return value is what they change of the class as the kernels keep it (toric: the four winding parities, which only
// an odd lattice's operators move -- an even L's rows and columns hold an even number of qubits; xzzx: the internal value of wu_stage_lds).
template <int CODE, class Row>
__host__ __device__ __forceinline__ uint32_t wu_logical(uint32_t A, uint32_t B, int L, Row &&row)
{
    if constexpr (CODE == kCodeToric) {
        const uint32_t op0 = (A >> 14) & 3u, op1 = (A >> 12) & 3u;
        const uint32_t dx0 = (op0 ^ (op0 >> 1)) & 1u, dz0 = op0 >> 1, dx1 = (op1 ^ (op1 >> 1)) & 1u, dz1 = op1 >> 1;
        if (dx0) row(0u, ((A & 0xFFFu) * (uint32_t)L) >> 12);
        if (dz0) row(1u, ((B >> 21) * (uint32_t)L) >> 11);
        if (dx1) row(2u, (((B >> 10) & 0x7FFu) * (uint32_t)L) >> 11);
        if (dz1) row(3u, ((B & 0x3FFu) * (uint32_t)L) >> 10);
        return (L & 1) ? dx0 | (dz0 << 1) | (dx1 << 2) | (dz1 << 3) : 0u;
    } else {
        const uint32_t op = (A >> 14) & 3u;
        const uint32_t hx = (op ^ (op >> 1)) & 1u, hz = op >> 1;
        const uint32_t xp = hx ? ((A & 0x3FFFu) * (uint32_t)L) >> 14 : 0u, zp = hz ? ((B >> 16) * (uint32_t)L) >> 16 : 0u;
        const uint32_t ax = CODE == kCodeXzzx ? hx : (op & 1u), az = hz;
        if (ax) row(0u, xp);
        if (az) row(1u, zp);
        return ax | (az << 1);
    }
}

// What one proposal of the top rung adds to the row of its step: xor_word(w, v) for w < WV is "mask word w ^= v", xor_word(WV, v) the class change.
// The proposal is a logical operator iff thr16 != 0 && A[31:16] < thr16 (thr16 = ceil(p_logical 2^16)), else the stabilizer g = floor(B G / 2^32), applied
// unseen: desc_word(g, i) is dword i of its descriptor (tables.hpp: toric_wave_descriptors, 8 dwords; wave_descriptors, 16), lml_word(kind, pos, w) word w of
// a row of the logical masks.  Words that are zero are left out (the masks of a row operator touch a few words of the state only).
template <int CODE, int WV, class Desc, class Lml, class Xor>
__host__ __device__ __forceinline__ void wu_frame_add(uint32_t A, uint32_t B, uint32_t thr16, uint32_t G, int L, Desc &&desc_word, Lml &&lml_word, Xor &&xor_word)
{
    if (thr16 != 0 && (A >> 16) < thr16) {
        // (one pass over the words for all kinds: a kind that does not act reads its identity row, position L -- lanes of a wavefront that hold
        // different operators then walk the same loop)
        uint32_t at[4] = {(uint32_t)L, (uint32_t)L, (uint32_t)L, (uint32_t)L};
        const uint32_t cd = wu_logical<CODE>(A, B, L, [&](uint32_t kind, uint32_t pos) { at[kind] = pos; });
#if defined(__clang__)
#pragma unroll 2
#endif
        for (int w = 0; w < WV; ++w) {
            uint32_t v = lml_word(0u, at[0], w) ^ lml_word(1u, at[1], w);
            if constexpr (CODE == kCodeToric) v ^= lml_word(2u, at[2], w) ^ lml_word(3u, at[3], w);
            if (v) xor_word((uint32_t)w, v);
        }
        if (cd) xor_word((uint32_t)WV, cd);
        return;
    }
    const uint32_t g = (uint32_t)(((uint64_t)B * G) >> 32);     // (philox.hpp scale_u32)
    if constexpr (CODE == kCodeToric) {
        // (the own-cell pair as one value, 5 P << s, then the other two sites)
        for (int u = 0; u < 3; ++u) xor_word(desc_word(g, u) & 0xFFu, desc_word(g, 3 + u));
    } else {
        for (int u = 0; u < 4; ++u) {
            const uint32_t v = desc_word(g, 4 + u);               // (a site that does not exist: 0)
            if (v) xor_word(desc_word(g, u) & 0xFFu, v);
        }
    }
}

// The rows of a whole pick window from its 64 pick blocks (picks[4 l .. 4 l + 3]: the words A, B of proposals 2l and 2l + 1, lane l's block) for `iters`
// proposals per step: frames[steps][WV + 1] with steps = 128 / iters, proposal P in row P / iters.  The host's form of what the top rung's wave does
// lane-parallel in wu_run's refresh (there with iters = 10 and LDS atomics); desc / lml as the plan uploads them, lml rows padded to WV words.
template <int CODE, int WV>
inline void wu_build_frames(const uint32_t *picks, uint32_t iters, uint32_t thr16, uint32_t G, int L, const uint32_t *desc, const uint32_t *lml, uint32_t *frames)
{
    const uint32_t steps = 128u / iters;
    for (uint32_t i = 0; i < steps * (uint32_t)(WV + 1); ++i) frames[i] = 0u;
    for (uint32_t P = 0; P < steps * iters; ++P) {
        const uint32_t *b = picks + 4u * (P >> 1) + 2u * (P & 1u);
        uint32_t *row = frames + (P / iters) * (uint32_t)(WV + 1);
        wu_frame_add<CODE, WV>(b[0], b[1], thr16, G, L,
                               [&](uint32_t g, int i) { return desc[(size_t)g * (CODE == kCodeToric ? 8u : 16u) + (uint32_t)i]; },
                               [&](uint32_t kind, uint32_t pos, int w) { return lml[((size_t)kind * (uint32_t)(L + 1) + pos) * (uint32_t)WV + (uint32_t)w]; },
                               [&](uint32_t w, uint32_t v) { row[w] ^= v; });
    }
}

}  // namespace qecmc
