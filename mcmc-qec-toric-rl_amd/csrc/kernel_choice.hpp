// Which kernel a ladder launch runs: the one place that decides it.  Host C++ only (like tables.hpp): capi.hip and the launch
// path (ladder_rs.hip) ask choose_kernel(), and tables_test_api.cpp builds it alone with g++ so that tests/test_kernel_choice.py can
// enumerate every shape the C-ABI accepts.  The LDS carve-ups the choice depends on live here too; the kernels include them from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "stencil_bytes.hpp"   // kCode* constants

namespace qecmc {

// The shortest-chain statistics (qecmc_plan_set_shortest; shortest_book.hpp) keep kShortRows words per ladder in LDS: per class c the minimum (low, high word of
// the double), shortest_n and the unique count at rows 4 c .. 4 c + 3, the distinct keys offered to the ladder's set at row 16, its overflow flag at row 17
constexpr int kShortRows = 18;
constexpr int kSwapFast = 64;       // swap-threshold entries per rung pair kept in LDS (d < kSwapFast)
constexpr uint32_t kMaxGenLds = 2048;   // generator tables up to this many entries are staged in LDS
constexpr int kLutTypes = 8;        // rows of the plaquette codes' dE look-up table (Pauli patterns of their generators; more: no table)
constexpr int kGenSplit = 255;      // ds_read2_b64's second offset is an 8-bit count of 8-byte units

// The variants of ladder_kernel<MAXT, MINW, CODE, FLAGS> (ladder_kernel.hpp describes each)
enum LadderFlag : uint32_t {
    kConv = 1u << 0, kGsplit = 1u << 1, kBiased = 1u << 2, kScan = 1u << 3, kGentop = 1u << 4, kUset = 1u << 5, kAlpha = 1u << 6,
    kPre = 1u << 7, kDelut = 1u << 8, kQueue = 1u << 9, kSsw = 1u << 10,
};

// ladder_kernel: dwords of one group (keep in sync with the kernel)
__host__ __device__ inline int ladder_group_dwords(int Nc, int W, int ncls, int gen_dwords)
{
    // st + info[2] + swx[2] + hist + thrT + swapT + stop flag (16) + generator table
    int d = Nc * W * 64 + 4 * Nc * 64 + ncls * 64 + Nc * 9 + Nc * kSwapFast + 16;
    d = (d + 3) & ~3;          // 16-byte aligned generator table (ds_read_b128 entries)
    return d + ((gen_dwords + 3) & ~3);
}
inline size_t ladder_stats_lds_bytes(int Nc) { return sizeof(uint32_t) * 64u * (size_t)(2 * Nc); }   // [Nc] swap accepts (row Nc-1 idle) + [Nc] error sums
// dwords of the LDS generator table: the toric random-scan kernels expand each generator to 4 x u32
// (byte offset << 16 | pauli fields | bit shift), the other paths keep the plan's 4 x u16 form.  Up to kGenSplit
// generators the expanded table is stored as two halves kGenSplit entries apart (sites 0,1 | sites 2,3).
// alpha noise appends the double-buffered n_eff records [2][Nc][64] to the region
// ... and the biased / alpha rules' count-change table uint2[n_types][256] and packed per-state counts uint32[Nc][64]
// lattice size of a plaquette code from its qubit count (xzzx / rotated: L x L; planar: 2 L^2 with an idle row and column)
inline int nq_L(int code, int nq) { int L = 1; while ((code == 3 ? 2 * L * L : L * L) < nq) ++L; return L; }
inline int ladder_gen_dwords(int code, int noise, int scan, uint32_t n_gen, int Nc, int nq = 0, int n_types = 0)
{
    // depolarizing random scan: the expanded table of the non-top proposal loop; the plaquette codes also keep the plan's
    // form for their top-chain / general paths
    const bool wide = !scan;                                   // (biased / alpha kernels: unsplit, next to the plan's form)
    // (toric, unsplit: 128 dwords behind the table for the dE look-up table, which the split form keeps between its halves)
    // (plaquette codes: 256 bytes per Pauli pattern behind their expanded table)
    const int lut_tail = noise ? 0 : code == 0 ? ((int)n_gen > kGenSplit ? 128 : 0) : 64 * kLutTypes;
    // (the xzzx / rotated / planar kernels are never built with kGsplit and carve 4 G dwords: this reserves the split size for them too)
    const int wide_dw = ((!noise && (int)n_gen <= kGenSplit) ? 2 * (kGenSplit + (int)n_gen) : 4 * (int)n_gen) + lut_tail;
    int d = wide ? (code == 0 ? wide_dw : ((2 * (int)n_gen + 3) & ~3) + wide_dw) : 2 * (int)n_gen;
    if (noise == 2) d = ((d + 3) & ~3) + 2 * Nc * 64;
    // (8 bytes per count-change entry; + the X / Z logical masks [2][L+1][W]; xzzx: + the logical operators' fields per generator)
    if (noise) d = ((d + 3) & ~3) + 512 * n_types + Nc * 64 + 2 * (nq_L(code, nq) + 1) * ((nq + 15) / 16) + (code == 1 ? (((int)n_gen + 1) & ~1) + 3 * 64 : 0);
    return d;
}
inline size_t ladder_lds_bytes(int Nc, int W, int ncls, int gen_dwords) { return sizeof(uint32_t) * (size_t)ladder_group_dwords(Nc, W, ncls, gen_dwords); }

// ladder_colour_kernel: LDS of one workgroup (dwords): states, records, swap uniforms, histogram, then the tables every phase reads -- the
// phase table, the generator table, the logical masks, the swap thresholds (32-bit where they fit) -- so that the serial path of a
// step never waits for global memory
// (noise != 0: the rule's 81 thresholds per rung; the alpha rule's n_eff records by step parity)
// (shortest: the shortest-chain statistics' state of the ladder, kShortRows words behind everything else)
inline size_t colour_lds_dwords(int Nc, int W, int ncls, uint32_t n_phases, uint32_t n_gen, int L, int nq, bool swap32, int noise = 0, bool shortest = false)
{
    return (size_t)Nc * W + 4 * (size_t)Nc + ncls + 32u * n_phases + 2u * n_gen + 4u * (L + 1) * W +
           (swap32 ? 1u : 2u) * (size_t)(Nc > 1 ? Nc - 1 : 0) * (nq + 1) + 2 + 4 +   // (+ 2: the stop flag by step parity)
           (noise ? (size_t)Nc * 81 + 2 * (size_t)Nc : 0) + (shortest ? (size_t)kShortRows : 0);
}
// ... and where that state starts (dwords; the alpha rule's kernel: ladder_colour_body.inc carves the regions in this order, the generator table 8-byte aligned)
__host__ __device__ inline uint32_t colour_short_at(int Nc, int W, int ncls, uint32_t n_phases, uint32_t n_gen, int L, int nq, bool swap32)
{
    const uint32_t head = (uint32_t)(Nc * W + 4 * Nc + ncls) + 32u * n_phases;
    return head + (head & 1u) + 2u * n_gen + 4u * (uint32_t)((L + 1) * W) + (swap32 ? 1u : 2u) * (uint32_t)((Nc > 1 ? Nc - 1 : 0) * (nq + 1)) + 2u +
           (uint32_t)Nc * 81u + 2u * (uint32_t)Nc;
}

// ladder_wu_kernel: LDS carve-up of one workgroup (dwords): the exchange buffer (W words per rung), records, swap uniforms, histogram, acceptance
// rows, swap rows, logical masks (rows padded to WV words, + 64: the frame reads a row with all 64 lanes), stop / refill flags, and -- the
// criterion kernels -- wave 0's per-ladder bookkeeping [kWuBk][64] and the refill mailbox [2][64]
struct WuLds { int xbuf, rec, swd, hist, thr, swapT, lml, stop, bk, mail, bot, cht, nef, lnb, bot2, skey, sst, frm, total; };
constexpr int kWuBk = 13;      // tops0, samples, burn, conv_start, conv_streak, sumA lo / hi, sumB lo / hi, state (done | pending << 1 | has << 3),
                               // steps_done, converged, the lane's ladder (QUEUE)
constexpr int kWuBkAlpha = 17; // ... and the alpha rule's second pair of window sums (n_x + n_y): sumAxy lo / hi, sumBxy lo / hi
__host__ __device__ inline int wu_words(int W) { return W <= 4 ? 4 : W <= 8 ? 8 : W <= 12 ? 12 : W <= 16 ? 16 : 32; }   // WV: state words per rung, padded
constexpr int kWuHalf = 16;                                                                               // rows per rung of a 32-word kernel's exchange buffer
// rows per rung of the exchange buffer.  The fixed-length kernels give a rung the kernel's padded width (16 per half of a 32-word state): the padding
// words travel with the rest (they are zero), so that no transfer tests the lattice's width at run time on the scalar unit, the busiest unit of these
// kernels (-30 tests per step at 29 words).  The criterion kernels keep the tight layout -- W rows, a transfer of a word at or beyond wu_words_min
// tests the width --: padded rows cost the headline shape's criterion kernel its fourth workgroup per CU (42 KB instead of 39.9) and the route 11 %.
__host__ __device__ inline int wu_rows(int W, bool conv) { return W > 16 ? kWuHalf : conv ? W : wu_words(W); }
// The fixed-length kernels of up to 16 words under the depolarizing rule with the unrolled proposal loop (it = 10) keep the top rung's moves of a pick
// window as frames (wu_frames.hpp): [steps][WV + 1] words behind everything else, private to the top rung's wave, steps = 128 / 10 ladder steps per
// window.  wu_frame_steps: that number for a kernel of these properties (`it` as in the kernel key: 10 or 0), 0 for a kernel without the buffer.
__host__ __device__ constexpr int wu_frame_steps(int wv, bool conv, bool alpha, int it) { return !conv && !alpha && wv <= 16 && it == 10 ? 128 / 10 : 0; }
// (alpha rule: the 9 x 9 table of a proposal's count change as two fp16 numbers, the slots' n_eff attributes as doubles [Nc][64], ln(pz_i / pz_i+1),
// and -- criterion runs -- slot 0's n_eff record by step parity; shortest: the key of rung 0's new state by step parity [2][2][64] beside it, and the
// booking wave's per-lane state of the shortest-chain statistics [kShortRows][64])
__host__ __device__ inline WuLds wu_lds(int Nc, int W, int ncls, int L, bool conv, bool alpha = false, bool shortest = false, int frame_steps = 0)
{
    const int WV = wu_words(W);
    WuLds o;
    o.xbuf = 0;
    o.rec = o.xbuf + Nc * wu_rows(W, conv) * 64;
    o.swd = o.rec + Nc * 64;
    o.hist = o.swd + Nc * 64;
    o.thr = o.hist + ncls * 64;               // [Nc][2][9]: high 13 / low 32 bits of ceil(f^dE 2^44), dE + 4 = 0 .. 8
    o.swapT = o.thr + Nc * 18;
    o.lml = o.swapT + Nc * kSwapFast;
    o.stop = o.lml + 4 * (L + 1) * WV + 64;
    o.bk = o.stop + 4;
    o.mail = o.bk + (conv ? (alpha ? kWuBkAlpha : kWuBk) * 64 : 0);   // [2][64] refill orders by step parity
    o.bot = o.mail + (conv ? 2 * 64 : 0);                    // [2][64] the record that landed in rung 0, by step parity
    o.cht = o.bot + (conv ? 2 * 64 : 0);
    o.nef = (o.cht + (alpha ? 84 : 0) + 1) & ~1;             // (doubles: 8-byte aligned)
    o.lnb = o.nef + (alpha ? Nc * 128 : 0);
    o.bot2 = o.lnb + (alpha ? 2 * Nc : 0);
    o.skey = o.bot2 + (alpha && conv ? 2 * 64 : 0);
    o.sst = o.skey + (shortest ? 4 * 64 : 0);
    o.frm = o.sst + (shortest ? kShortRows * 64 : 0);
    o.total = o.frm + frame_steps * (WV + 1);
    return o;
}
inline size_t wu_lds_bytes(int Nc, int W, int ncls, int L, bool conv, bool alpha, bool shortest = false, int frame_steps = 0)
{
    return sizeof(uint32_t) * (size_t)wu_lds(Nc, W, ncls, L, conv, alpha, shortest, frame_steps).total;
}
// ... of the kernel choose_wave picks for a launch of `iters` proposals per step (statistics launches run the general loop and ask for less: ladder_rs.hip)
inline size_t wu_plan_lds_bytes(int Nc, int W, int ncls, int L, bool conv, bool alpha, int iters)
{
    return wu_lds_bytes(Nc, W, ncls, L, conv, alpha, false, wu_frame_steps(wu_words(W), conv, alpha, iters == 10 ? 10 : 0));
}

// What the choice reads of a launch (kernel_shape(LadderArgs), plan_host.hpp).  top_acc / lower_acc: the top rung / some rung below it accepts every
// proposal (acc_all_mask); logical: thr_logical != 0; queue: a work queue is offered (a.queue; plan_host() asks with 1 whether a plan takes one);
// uset / xyz / stats / neff: a.uset_tab / a.xyz_thr / a.swap_acc / a.neff given (stats = 2: a.short_neff given instead, the shortest-chain statistics); f32ok: every rung below the top may take the single-precision
// acceptance estimate (bias_f32ok); tune: the developer bits of qecmc_params.flags (include/qecmc.h qecmc_flag)
struct KernelShape {
    int code, noise, scan, L, Nc, W, nq, ncls, n_gen, n_types, gen_type, top_acc, lower_acc, logical, conv, queue, uset, xyz, stats, resume, neff, f32ok,
        swap_fast_ok, iters, tune;
};

// The kernel a shape runs: ladder_kernel<maxt, minw, code, flags>, ladder_wu_kernel<maxt, minw, code, wv, conv, queue = conv, it, alpha> or
// ladder_colour_kernel<code, conv, rule, maxt, minw> -- with flags = kKeyStats in the wave / colour families: ladder_wu_stats_kernel<code, wv, alpha> or
// ladder_colour_stats_kernel<code, rule> --; family kRefused: no kernel is built for the shape (`why` names the rule)
enum KernelFamily : int { kRefused = 0, kFamLadder = 1, kFamWave = 2, kFamColour = 3 };
struct KernelKey {
    int family, maxt, minw, code;
    uint32_t flags;
    int wv, conv, it, alpha, rule;
    const char *why;
    bool ok() const { return family != kRefused; }
    bool takes_queue() const { return family == kFamLadder ? (flags & kQueue) != 0 : family == kFamWave && conv; }   // (scan = wave: its own queue)
    bool operator==(const KernelKey &o) const
    {
        return family == o.family && maxt == o.maxt && minw == o.minw && code == o.code && flags == o.flags && wv == o.wv && conv == o.conv && it == o.it &&
               alpha == o.alpha && rule == o.rule;
    }
};
inline KernelKey refuse(const char *why) { return {kRefused, 0, 0, 0, 0u, 0, 0, 0, 0, 0, why}; }
inline KernelKey ladder_key(int maxt, int minw, int code, uint32_t flags) { return {kFamLadder, maxt, minw, code, flags, 0, 0, 0, 0, 0, nullptr}; }
inline KernelKey wave_key(int maxt, int minw, int code, int wv, bool conv, int it, bool alpha) { return {kFamWave, maxt, minw, code, 0u, wv, conv, it, alpha, 0, nullptr}; }
inline KernelKey colour_key(int code, bool conv, int rule) { return {kFamColour, 1024, 4, code, 0u, 0, conv, 0, 0, rule, nullptr}; }
// The statistics kernels of the wave and colour families (qecmc_plan_set_stats: ladder_wu_stats_kernel<code, wv, alpha>, ladder_colour_stats_kernel<code,
// rule>): kernels of their own, told from the fast ones by `flags` -- 0 in both families otherwise.  Fixed-length runs, 1 024 threads at 4 waves per SIMD
// whatever the ladder's length, the general proposal loop (it = 0).
constexpr uint32_t kKeyStats = 1u;
inline KernelKey wave_stats_key(int code, int wv, bool alpha) { return {kFamWave, 1024, 4, code, kKeyStats, wv, 0, 0, alpha, 0, nullptr}; }
inline KernelKey colour_stats_key(int code, int rule) { return {kFamColour, 1024, 4, code, kKeyStats, 0, 0, 0, 0, rule, nullptr}; }

// The shortest-chain kernels (qecmc_plan_set_shortest: ladder_wu_shortest_kernel<code, wv, it>, ladder_colour_shortest_kernel<code>): the alpha rule's criterion
// kernels with the per-class minimum of slot 0's n_eff attribute and the set of distinct configurations seen at it -- kernels of their own again, flags =
// kKeyShort.  They serve conv_mode NONE too (the criterion is then never consulted), so `conv` is 1 in their keys whatever the launch's.
constexpr uint32_t kKeyShort = 2u;
inline KernelKey wave_short_key(int code, int wv, int it) { return {kFamWave, 1024, 4, code, kKeyShort, wv, 1, it, 1, 0, nullptr}; }
inline KernelKey colour_short_key(int code) { return {kFamColour, 1024, 4, code, kKeyShort, 0, 1, 0, 0, 2, nullptr}; }

// dynamic LDS of a ladder_kernel workgroup (+ the per-lane statistics counters behind the group's region)
inline size_t ladder_launch_lds(const KernelShape &s)
{
    return ladder_lds_bytes(s.Nc, s.W, s.ncls, ladder_gen_dwords(s.code, s.noise, s.scan, s.n_gen, s.Nc, s.nq, s.n_types)) + (s.stats ? ladder_stats_lds_bytes(s.Nc) : 0);
}
// PRE (the top chain's Philox blocks drawn ahead: 105-119 VGPRs, 4 waves per SIMD) for ladders of up to 8 rungs whose LDS footprint leaves a CU at most
// two workgroups anyway.  (A longer ladder would get ONE: toric L = 9, Nc = 9 / 12 / 16 measured 0.31 / 0.39 / 0.44 with PRE against 0.37 / 0.59 / 0.45.)
inline bool ladder_wants_pre(const KernelShape &s) { return s.Nc >= 3 && s.Nc * 64 <= 512 && 3 * ladder_launch_lds(s) > 160 * 1024 && s.logical && !(s.tune & 2); }
// a criterion run offered a work queue takes it: depolarizing rule, random scan, the framed top chain (toric L <= 16, plaquette codes L <= 32; a top
// rung at p = 0.75, i.e. Nc >= 2, with logical moves) ... and the biased / alpha rules on the xzzx / rotated codes (any L, Nc)
inline bool ladder_takes_queue(const KernelShape &s)
{
    if (!s.queue || s.scan || !s.conv || s.uset) return false;
    return s.noise ? s.code == kCodeXzzx || s.code == kCodeRotated : s.L <= (s.code == kCodeToric ? 16 : 32) && s.Nc >= 2 && s.logical;
}

// the toric code, depolarizing rule, the reference's random scan: the headline kernel family
inline KernelKey choose_ladder_toric(const KernelShape &s)
{
    const bool big = s.Nc * 64 > 512;                    // 9 .. 16 rungs: 1024-thread workgroups at 4 waves per SIMD
    // the general top-chain path is needed only for L > 16 or a top chain below p = 0.75 (1-chain ladder)
    const bool gentop = s.logical && (s.L > 16 || !s.top_acc);
    const bool gsplit = s.n_gen <= kGenSplit;            // the table layout of ladder_gen_dwords()
    const size_t lds = ladder_launch_lds(s);
    // the dE look-up table (DELUT): between the halves of a split table (L <= 9) or behind an unsplit one (L >= 12), ladder_gen_dwords
    // (three workgroups per CU -- L = 10 ... 12 at 8 temperatures -- are the LDS-bound shapes: -1.5 % with the table)
    const bool lut = !(s.tune & 4) && (!gsplit || s.n_gen + 64 <= kGenSplit) && (160 * 1024) / lds != 3;
    uint32_t want = (s.conv ? kConv : 0u) | (gsplit ? kGsplit : 0u);
    if (s.queue) {
        if (gentop) return refuse("toric work queue: no general top-chain path");
        want |= kQueue | ((!big && gsplit && s.n_gen + 64 <= kGenSplit) ? kDelut : 0u);
    } else if (gentop) {
        want |= kGentop;
    } else if (ladder_wants_pre(s)) {
        return ladder_key(512, 4, kCodeToric, want | kPre | (lut ? kDelut : 0u));
    } else if (!s.conv && !big && 4 * lds <= 160 * 1024 && !(s.tune & 8) && gsplit) {
        want |= kSsw | (lut ? kDelut : 0u);              // the swap sweep run once by wave 0 (SSW) pays where four workgroups share a CU
    } else if (lut) {
        want |= kDelut;
    }
    return big ? ladder_key(1024, 4, kCodeToric, want) : ladder_key(512, 8, kCodeToric, want);
}

// xzzx, rotated and planar codes, depolarizing rule, random scan: always the table-driven general top-chain path
inline KernelKey choose_ladder_surf(const KernelShape &s)
{
    const bool big = s.Nc * 64 > 512;
    const size_t lds = ladder_launch_lds(s);
    // dE of a proposal from the look-up table behind the expanded generator table (DELUT, one row per Pauli pattern)
    // (measured: +8 % xzzx L = 9, +7.7 % rotated L = 9, +5.6 % rotated L = 13, +1 % planar L = 9 -- four workgroups per CU, bound by VALU
    // issue; 0 % rotated L = 21 -- two; -4 % xzzx L = 15 -- three per CU, where the LDS pipe is the busier one)
    const bool lut = !(s.tune & 4) && s.gen_type && s.n_types > 0 && s.n_types <= kLutTypes && (160 * 1024) / lds != 3;
    uint32_t want = kGentop | (s.conv ? kConv : 0u);
    if (s.queue) {
        if (!s.top_acc) return refuse("plaquette-code work queue: no top chain below p = 0.75");   // (built on the blind top chain)
        want |= kQueue;
    } else if (ladder_wants_pre(s) && s.top_acc) {       // (the blind path is what the blocks drawn ahead feed)
        return ladder_key(512, 4, s.code, want | kPre | (lut ? kDelut : 0u));
    } else if (!s.conv && !big && 4 * lds <= 160 * 1024 && !(s.tune & 8)) {
        want |= kSsw | (lut ? kDelut : 0u);
    } else if (lut) {
        want |= kDelut;
    }
    return big ? ladder_key(1024, 4, s.code, want) : ladder_key(512, 8, s.code, want);
}

// the biased (src/mcmc_biased.py) and alpha (src/mcmc_alpha.py) acceptance rules on the xzzx / rotated codes
inline KernelKey choose_ladder_biased(const KernelShape &s)
{
    if (s.code != kCodeXzzx && s.code != kCodeRotated) return refuse("biased / alpha rule: xzzx and rotated codes only");
    const bool big = s.Nc * 64 > 512;
    uint32_t want = kBiased | kGentop | (s.conv ? kConv : 0u) | (s.noise == 2 ? kAlpha : 0u);
    // (the queue kernels carry the criterion's window sums, the refill state and the biased rule's counts: at 64 VGPRs they would
    // spill 130-250 B per lane into their hot loops, so they run at 128 VGPRs / 4 waves per SIMD whatever the workgroup size)
    if (s.queue) return ladder_key(big ? 1024 : 512, 4, s.code, want | kQueue);
    if (!big && !s.conv && 4 * ladder_launch_lds(s) <= 160 * 1024 && !(s.tune & 8)) want |= kSsw;
    return big ? ladder_key(1024, 4, s.code, want) : ladder_key(512, 8, s.code, want);
}

// scan = 1: the systematic generator sweep (depolarizing rule, every code; toric: the general top-chain path as on the random scan)
inline KernelKey choose_ladder_sweep(const KernelShape &s)
{
    const bool gentop = s.code != kCodeToric || (s.logical && (s.L > 16 || !s.top_acc));
    const uint32_t want = kScan | (s.conv ? kConv : 0u) | (gentop ? kGentop : 0u);
    return s.Nc * 64 > 512 ? ladder_key(1024, 4, s.code, want) : ladder_key(512, 8, s.code, want);
}

// the unique-chain set insertion of PTDC / STDC / PTRC / STRC (direct counting)
inline KernelKey choose_ladder_uset(const KernelShape &s)
{
    if ((s.noise && s.noise != 2) || s.scan || s.conv || s.logical) return refuse("uset: depolarizing or alpha rule, random scan, fixed length, no logical moves");
    if (s.xyz && (s.code == kCodeToric || s.Nc != 1 || s.noise)) return refuse("uset: Chain_xyz runs single chains of the table-driven codes");
    if (s.noise == 2) {   // STDC_droplet_alpha (decoders.py:510-534)
        if (s.Nc != 1 || (s.code != kCodeXzzx && s.code != kCodeRotated)) return refuse("uset, alpha rule: single chains of the xzzx / rotated codes");
        return ladder_key(1024, 4, s.code, kUset | kBiased | kAlpha | kGentop);
    }
    const uint32_t want = kUset | (s.n_gen <= kGenSplit ? kGsplit : 0u);
    return s.Nc * 64 > 512 ? ladder_key(1024, 4, s.code, want) : ladder_key(512, 8, s.code, want);
}

// scan = 2: one workgroup of 1 024 threads at 4 waves per SIMD per ladder, whatever its length (512 threads at 6 or 8 waves per SIMD:
// profiles/r04_colour_occupancy_ab.json)
inline KernelKey choose_colour(const KernelShape &s)
{
    if (s.uset) return refuse("uset: not with scan = colour");
    if (s.noise < 0 || s.noise > 2 || s.resume) return refuse("scan = colour: no resumed ladders");
    if (s.noise != 0 && s.code != kCodeXzzx && s.code != kCodeRotated) return refuse("biased / alpha rule: xzzx and rotated codes only");
    if (s.stats) {   // qecmc_plan_set_stats: a wave per slot counts its own pair and its slot's errors
        if (s.conv) return refuse("scan = colour: swap statistics are collected in fixed-length runs only, not with the criterion");
        if (s.Nc < 2) return refuse("swap statistics need Nc >= 2");
        return colour_stats_key(s.code, s.noise);
    }
    return colour_key(s.code, s.conv, s.noise);
}

// scan = 3 (ladder_wu.hpp): the depolarizing rule with a top rung that accepts every move (Nc >= 2, p_top = 0.75) and rungs at distinct
// temperatures, up to 16 state words per rung (toric / planar L <= 11, xzzx / rotated L <= 16), fixed-length runs of up to 8 rungs also up to 32
// (toric L <= 16, xzzx / rotated L <= 22); the alpha rule (top rung at pz_tilde = 1) on the xzzx / rotated codes up to 8 words, where every rung
// below the top may take the single-precision acceptance estimate; 1 <= iters <= 128.  (Statistics, s.stats: choose_wave answers for them.)
inline bool wu_supported(const KernelShape &s)
{
    if (s.noise == 2)
        return (s.code == kCodeXzzx || s.code == kCodeRotated) && s.Nc >= 2 && s.Nc <= 16 && s.W <= 8 && s.n_gen <= 1023 && s.iters >= 1 && s.iters <= 128 &&
               s.f32ok && !s.uset && !s.resume && !s.neff && wu_plan_lds_bytes(s.Nc, s.W, s.ncls, s.L, s.conv, true, s.iters) <= 160 * 1024;
    return s.noise == 0 && s.Nc >= 2 && s.top_acc && !s.lower_acc && (s.W <= 16 || (s.W <= 32 && !s.conv && s.Nc <= 8 && s.code != kCodePlanar)) &&
           s.n_gen <= 1023 && s.iters >= 1 && s.iters <= 128 && s.swap_fast_ok && !s.uset && wu_plan_lds_bytes(s.Nc, s.W, s.ncls, s.L, s.conv, false, s.iters) <= 160 * 1024;
}
// the padded state width (wu_words); 8 waves per SIMD up to 12 words, 6 at 16 and 32 words and for the alpha rule's criterion kernels (scratch
// reloaded every step at 8: profiles/r04_crit_occupancy_ab.json); 9 .. 16 rungs: the same code under a launch bound of 1 024 threads; IT = 10: the
// unrolled proposal loop of iters = 10 (decoders.py:25); conv: the criterion kernel on its persistent grid, with its own work queue
inline KernelKey choose_wave(const KernelShape &s)
{
    if (!wu_supported(s)) return refuse("scan = wave: outside what it is built for");
    const int maxt = s.Nc * 64 > 512 ? 1024 : 512, it = s.iters == 10 ? 10 : 0, wv = wu_words(s.W);
    if (s.stats) {   // qecmc_plan_set_stats: the kernels with the two counters per wave (ladder_wu.hpp STATS)
        if (s.conv) return refuse("scan = wave: swap statistics are collected in fixed-length runs only, not with the criterion");
        if (wv > 16) return refuse("scan = wave: no swap statistics above 16 state words per rung (the 32-word kernels' staging spills)");
        return wave_stats_key(s.code, wv, s.noise == 2);
    }
    if (s.noise == 2) return wave_key(maxt, s.conv ? 6 : 8, s.code, wv, s.conv, it, true);
    return wave_key(maxt, wv <= 12 ? 8 : 6, s.code, wv, s.conv, it, false);
}

// scan = 3: who walks the swap cascade of a step (ladder_wu.hpp, the lean step tail).  true: the top rung's wave once for the workgroup, its result handed to the other waves behind a third barrier; false: every wave replays it down to its own rung.  Not part of the
// kernel key: both forms live in the one kernel behind a wave-uniform test of LadderArgs::wu_once, which the launch sets from here.  Where ladder_kernel's
// SSW variant would be eligible (choose_ladder_toric: fixed length, depolarizing rule, at most 16 words, workgroups of up to 512 threads of which four fit
// a CU -- the serial section is covered by the CU's other workgroups) the measurement decides, and it turns on the ladder's length alone, whatever the code
// and the state width.  wave_cascade_once() is the record of the PLAIN once form -- the waves below the top idle between the second and the
// third barrier --: it gained 2.6 - 5.2 % at 5, 6 and 7 rungs and lost 0.5 - 3.8 % at 2, 3, 4 (too few replays to pay for the barrier) and, on the kernel of
// that day, at 8.  tests/test_wave_cascade_choice.py pins it answer by answer.  What a launch asks is wave_cascade_walk() below, which adds eight rungs for
// the kernels that draw ahead in the wait: re-measured on today's kernel the once form gains there too (42.66 -> 41.06 ms plain, 40.20 with
// the draw), so nothing about eight rungs is left unexplained or lost.
// QECMC_FLAG_NO_SSW (tune & 8): the replay.
// A statistics launch (flags = kKeyStats) always replays: its waves count the pair each of them decides.
inline bool wave_cascade_eligible(const KernelShape &s)
{
    const KernelKey k = choose_wave(s);
    return s.scan == 3 && k.ok() && k.flags == 0 && !k.conv && !k.alpha && k.wv <= 16 && s.Nc * 64 <= 512 && !(s.tune & 8) &&
           4 * wu_plan_lds_bytes(s.Nc, s.W, s.ncls, s.L, false, false, s.iters) <= 160 * 1024;
}
inline bool wave_cascade_once(const KernelShape &s) { return wave_cascade_eligible(s) && s.Nc >= 5 && s.Nc <= 7; }

// What the launch puts into LadderArgs::wu_once.  With the waves below the top drawing the next step's acceptance block in the wait for the third
// barrier (ladder_wu.hpp AHEAD: the kernels with the unrolled loop of iters = 10), the once form is a different program from the one
// wave_cascade_once() was measured on, so the ladder lengths it serves are a rule of their own: everything wave_cascade_once() says yes to, and eight rungs
// (config 2's ladder) where the shape is eligible in the same sense and the kernel draws ahead -- because the same-box A/B of the two forms says so
// (kWalkAtEightRungs; DESIGN.md 4.1g, profiles/r13_wave_walk_ab.json: config 2 42.66 -> 40.20 ms walked once, 42.56 replayed; the plain once form
// on today's kernel 41.06).  Two functions because the first is a measured record that tests pin, and this one is the choice.
constexpr bool kWalkAtEightRungs = true;
inline bool wave_cascade_walk(const KernelShape &s)
{
    if (wave_cascade_once(s)) return true;
    return kWalkAtEightRungs && s.Nc == 8 && s.iters == 10 && wave_cascade_eligible(s);
}

// The form of the walk (LadderArgs::wu_once: 0 the replay, 1, 2).  In the kernels whose top rung's wave draws both blocks of swap uniforms (ladder_wu.hpp
// TOPDRAWS: the frame kernels -- fixed length, depolarizing rule, at most 16 words, iters = 10 -- of up to 8 rungs) that wave was the last of its workgroup at
// the step's first barrier by the bounds it found behind the draw.  Form 2 spreads them: the top wave draws the NEXT step's words and hands them over raw
// behind its walk, and each wave below the top turns the word of the pair above its own slot into the bound.  Form 1 is the walk as it was.  The ladder
// lengths of form 2 are the ones at which the same-box A/B of the two forms had it ahead by the project's bar (kSpreadRungs, bit Nc;
// profiles/r15_wave_spread_ab.json): eight rungs -- config 2 39.85 -> 38.97 ms, 9.5 times the larger spread -- and no other: at 5, 6 and 7
// rungs form 2 lost 2.1, 1.0 and 1.2 % (the top wave is not the late one there).  QECMC_FLAG_NO_SPREAD (tune & 16): form 1 wherever form 2 would run.
constexpr uint32_t kSpreadRungs = 1u << 8;
inline int wave_cascade_mode(const KernelShape &s)
{
    if (!wave_cascade_walk(s)) return 0;
    const bool topdraws = s.Nc <= 8 && wu_frame_steps(wu_words(s.W), s.conv != 0, s.noise == 2, s.iters == 10 ? 10 : 0) != 0;
    return topdraws && ((kSpreadRungs >> s.Nc) & 1u) && !(s.tune & 16) ? 2 : 1;
}

// stats = 2, the shortest-chain statistics of PTEQ_alpha_with_shortest: a chooser of their own (no shape the sweeps of stats = 0 / 1 present comes here).
// The alpha rule on scan = wave -- what wu_supported() takes of it as a criterion run, on 1 024 threads at 4 waves per SIMD whatever the ladder's length --
// and on scan = colour under choose_colour's alpha conditions.
inline KernelKey choose_shortest(const KernelShape &s)
{
    if (s.noise != 2) return refuse("shortest-chain statistics: the alpha rule only (PTEQ_alpha_with_shortest)");
    if (s.scan != 2 && s.scan != 3) return refuse("shortest-chain statistics: scan = wave or scan = colour (scan = random: the host loop of PTEQ_alpha_with_shortest)");
    if (s.resume) return refuse("shortest-chain statistics: no resumed ladders");
    if (s.uset) return refuse("shortest-chain statistics: not with the unique-chain estimators' set");
    if (s.code != kCodeXzzx && s.code != kCodeRotated) return refuse("biased / alpha rule: xzzx and rotated codes only");
    if (s.scan == 2) return colour_short_key(s.code);
    KernelShape c = s;
    c.conv = 1; c.stats = 0;
    if (!wu_supported(c) || wu_lds_bytes(s.Nc, s.W, s.ncls, s.L, true, true, true) > 160 * 1024) return refuse("scan = wave: outside what it is built for");
    return wave_short_key(s.code, wu_words(s.W), s.iters == 10 ? 10 : 0);
}

// the kernel a launch of this shape runs, or why none is built for it
inline KernelKey choose_kernel(const KernelShape &s)
{
    if (s.stats == 2) return choose_shortest(s);
    if (s.scan == 3) return choose_wave(s);
    if (s.scan == 2) return choose_colour(s);
    // (a plain kernel never runs on the capped grid of a work queue)
    if (s.queue && !ladder_takes_queue(s)) return refuse("work queue offered to a shape without queue kernels");
    if (s.uset) return choose_ladder_uset(s);
    if (s.noise) return s.scan ? refuse("the sweep is built for the depolarizing rule only") : choose_ladder_biased(s);
    if (s.scan) return choose_ladder_sweep(s);
    return s.code == kCodeToric ? choose_ladder_toric(s) : choose_ladder_surf(s);
}

}  // namespace qecmc
