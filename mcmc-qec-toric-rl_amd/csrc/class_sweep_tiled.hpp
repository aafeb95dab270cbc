// The frontier sweep of class_sweep.hpp on a state vector that lives in HBM and passes through LDS one tile at a time: what reaches the shapes whose
// frontier is wider than an LDS state vector and too wide to hold down to one (rotated L = 13 .. 21, planar L = 8 .. 12, the toric code at L = 7).
//
// THE PLAN (build_tiled_plan).  The op stream is build_stream()'s, the one build_plan_held() encodes -- the same qubit order, INTRO just before first
// use, FORGET when closed, the lowest free slot first -- over a state vector A[2^width] of doubles, width <= hbm_width <= kTiledMaxWidth = 24 (128 MiB
// per class and assignment).  Where the frontier is wider than hbm_width generators are held out by build_cut_plan()'s rule unchanged: at the first
// peak, the live generator with the longest lifetime, ties to the lowest table index, until the width is <= hbm_width; kMaxHeld of them at most.  The
// held generators are summed over as class_sweep_cut.hpp sums them: one partial per assignment h, then cut_reduce().
//
// THE WIDE ENCODING.  The four-word ops of class_sweep.hpp keep a slot in 4 bits and the mask in 16; they are not changed.  Here one op is
//     [0]  kind | slot << 4 | pairs << 9 | top << 12      slot in 5 bits, pairs in 3, top in 5
//     [1]  mask, 32 bits: the occupied slots -- INTRO before it, CLOSE as they are, FORGET after it
//     [2]  CLOSE: four bytes (slot | xz << 5); bytes beyond `pairs` are 0
//     [3]  CLOSE: the qubit
//
// SEGMENTS.  A segment is a run of consecutive ops whose INTRO and FORGET slots all lie in one set T of tile_width index bits; CLOSE is diagonal and
// fits any T.  Within a segment the bits outside T are fixed: a TILE is one assignment of them, 2^tile_width entries, and the ops of the segment
// never carry a value from one tile to another.  So a workgroup gathers a tile into LDS, runs the whole segment there and writes the tile back: the
// state vector moves through HBM once per segment, not once per op.  The occupied slots outside T do not change within a segment (only INTRO and
// FORGET change them, and those are in T), so a tile is live for the whole segment or not at all: the live tiles are the 2^|live & ~T| assignments of
// the occupied fixed slots, and only those are launched.  The table is built greedily -- a segment is extended while its slots fit -- with the low
// kTileLowBits = 4 index bits always in T (3 at tile_width 4, which would otherwise leave no bit to choose): a tile then lies in HBM in runs of 16
// doubles, 128 bytes.  T is filled up to tile_width bits with the lowest bits it lacks, below state_bits = max(width, tile_width).
//
// ARITHMETIC.  Every entry sees the stream's fixed sequence of copies, single multiplies and single adds whatever the tiling: moving an entry between
// HBM and LDS is a copy.  The twin (sweep_tiled_host) is a plain loop over the wide stream, then cut_reduce(); the kernels (class_sweep_tiled.hip)
// agree with it bit for bit for every tile_width.  With nothing held and width <= 13 the result is qecmc_class_sweep's bit for bit, and where the holds
// are qecmc_class_sweep_cut's (hbm_width = its lds_width) it is that one's.  Both sides are built with -ffp-contract=off, without fast-math and without
// flush-to-zero: at L = 21 single entries reach the denormals, and host and device both keep them (tests/test_gpu_class_law_range.py feeds every
// sum-product kernel class weights below 2^-1022, down to 0: device and twin agree bit for bit there, class_sweep.hip and class_sweep_cut.hip,
// which are built without the two flags, included).
//
// DIRTY MEMORY.  Neither the workspace in HBM nor LDS is cleared.  The invariant: a live entry is always written by the INTRO that made it live
// before anything reads it.  A gather reads exactly the entries live at the segment's first op, and each of those was live at the end of the segment
// before, whose write-back stores exactly the entries live after its last op -- its tile was launched, being live.  The first segment reads nothing
// (it sets A[0] = 1), the last one stores its one live entry as the partial.
//
// Refused, before a device is looked for: QECMC_ERR_INVALID for a (code, L) check_code_L() does not know, a tile_width outside 4 .. 13 or an
// hbm_width outside tile_width .. 24 (0: the default of either, 11 and 24); QECMC_ERR_UNSUPPORTED for a (code, L) without a class move (the toric
// code at even L) and for a frontier that kMaxHeld held generators do not bring down to hbm_width, by name with its widths -- at the default, the toric
// code from L = 9 on (37 generators wide), the planar code from L = 13 and xzzx / rotated from L = 23 (26 wide everywhere: 12 holds leave 25 and 26).
#pragma once
#include "class_sweep_cut.hpp"

namespace qecmc {
namespace sweep {

constexpr int kTiledMaxWidth = 24;                  // the state vector of one (class, assignment): 2^24 doubles, 128 MiB
constexpr int kTileMinWidth = 4, kTileMaxWidth = kMaxWidth;     // a tile is an LDS state vector: 64 KiB at most, two workgroups per CU
constexpr int kTileDefaultWidth = 11;               // 16 KiB, 256 lanes, eight workgroups per CU: measured the fastest of 10 .. 13 at every shape
constexpr int kTileLowBits = 4;                     // 16 doubles = 128 bytes: the shortest run of a tile in HBM
constexpr size_t kTiledWorkspaceBytes = size_t(1) << 30;    // the state vectors of one pass
constexpr uint32_t kTiledUnitsMax = 65535;          // (class, assignment, syndrome) units of one pass: the y extent of a grid
constexpr int kTiledOpWords = 4, kTiledDevOpWords = 5, kSegmentWords = 8;
static_assert(kTiledMaxWidth <= 31 && kTileMaxWidth <= 16 && kTileMinWidth > 1, "a wide slot has 5 bits; a slot within a tile has 4");
static_assert((size_t(8) << kTiledMaxWidth) <= kTiledWorkspaceBytes, "one state vector fits the workspace");

// One segment of the host table (kSegmentWords words as tests read them): its ops, its tile bits T, every slot occupied at some op of it, the slots
// occupied before its first and after its last op, and the number of live tiles, 2^|live & ~T|
struct Segment {
    uint32_t op_first = 0, op_count = 0, tile = 0, live = 0, live_in = 0, live_out = 0, n_tiles = 0, pad = 0;
};

struct TiledPlan {
    Plan plan;                         // the header, the class-move table, rank and scale; plan.ops stays empty (the stream is in `ops`); refusal: the tiled plan's
    int hbm_width = 0, tile_width = 0, full_width = 0, n_held = 0, state_bits = 0;
    std::vector<int> held;             // table indices, ascending
    std::vector<uint32_t> held_words;  // [n_held][W]
    std::vector<uint32_t> ops;         // [n_ops][kTiledOpWords]: the wide encoding
    std::vector<Segment> segments;
    std::vector<uint32_t> dev_ops;     // [n_ops][kTiledDevOpWords]: every op in the coordinates of its segment's tile (below)
};

__host__ __device__ inline uint32_t popcount32(uint32_t v) { uint32_t n = 0; for (; v; v &= v - 1u) ++n; return n; }
// the bits of v at the positions of m, packed; and packed bits v spread to the positions of m
__host__ __device__ inline uint32_t bits_extract(uint32_t v, uint32_t m)
{
    uint32_t out = 0, k = 0;
    for (; m; m &= m - 1u, ++k) out |= ((v >> popcount32((m & (0u - m)) - 1u)) & 1u) << k;
    return out;
}
__host__ __device__ inline uint32_t bits_deposit(uint32_t v, uint32_t m)
{
    uint32_t out = 0;
    for (; m; m &= m - 1u, v >>= 1) out |= (0u - (v & 1u)) & (m & (0u - m));
    return out;
}

inline uint32_t wide_before(const uint32_t *op) { return (op[0] & 15u) == kForget ? op[1] | (1u << ((op[0] >> 4) & 31u)) : op[1]; }
inline uint32_t wide_after(const uint32_t *op) { return (op[0] & 15u) == kIntro ? op[1] | (1u << ((op[0] >> 4) & 31u)) : op[1]; }

// The device form of an op, in the coordinates of a tile of its segment (local bit k is the k-th lowest bit of T):
//     [0]  kind | local slot << 4 | local top << 8
//     [1]  the local mask
//     [2]  CLOSE: the pairs whose slot is in T, four bytes (local slot | xz << 4), 0 beyond them
//     [3]  CLOSE: the qubit
//     [4]  CLOSE: the pairs whose slot is fixed in the tile, four bytes (slot | xz << 5), 0 beyond them (xz is never 0): the tile's own bits decide them
inline void encode_dev_op(const uint32_t *op, uint32_t T, uint32_t *out)
{
    const uint32_t kind = op[0] & 15u, slot = (op[0] >> 4) & 31u, pairs = (op[0] >> 9) & 7u;
    const uint32_t lslot = kind == kClose ? 0u : popcount32(T & ((1u << slot) - 1u)), lmask = bits_extract(op[1], T);
    const uint32_t reach = kind == kClose ? lmask : lmask | (1u << lslot);
    uint32_t top = 0, local = 0, fixed = 0, nl = 0, nf = 0;
    while (top < 32u && (reach >> top)) ++top;
    for (uint32_t j = 0; j < pairs; ++j) {
        const uint32_t pr = (op[2] >> (8 * j)) & 0xFFu, s = pr & 31u, xz = pr >> 5;
        if ((T >> s) & 1u) local |= (popcount32(T & ((1u << s) - 1u)) | (xz << 4)) << (8 * nl++);
        else fixed |= (s | (xz << 5)) << (8 * nf++);
    }
    out[0] = kind | (lslot << 4) | (top << 8); out[1] = lmask; out[2] = local; out[3] = op[3]; out[4] = fixed;
}

inline TiledPlan build_tiled_plan(int code, int L, int hbm_width, int tile_width)
{
    TiledPlan tp;
    Plan &p = tp.plan;
    p.code = code; p.L = L;
    if (tile_width == 0) tile_width = kTileDefaultWidth;
    if (tile_width < kTileMinWidth || tile_width > kTileMaxWidth) {
        p.refusal = refuse_params(QECMC_ERR_INVALID, "tile_width=%d: the width of a tile in LDS is %d .. %d, or 0 for the default", tile_width, kTileMinWidth, kTileMaxWidth);
        return tp;
    }
    if (hbm_width != 0 && (hbm_width < tile_width || hbm_width > kTiledMaxWidth)) {
        p.refusal = refuse_params(QECMC_ERR_INVALID, "hbm_width=%d: the width of the state vector in HBM is tile_width = %d .. %d, or 0 for the default", hbm_width, tile_width,
                                  kTiledMaxWidth);
        return tp;
    }
    if (hbm_width == 0) hbm_width = kTiledMaxWidth;
    tp.hbm_width = hbm_width; tp.tile_width = tile_width;
    Trace tr;
    std::vector<char> held;
    Stream st = build_stream(code, L, held, &tr);
    p = st.head;
    tp.full_width = p.width;
    if (p.refusal.code) return tp;
    if (tp.full_width - kMaxHeld > hbm_width) {
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "the frontier of code %d at L=%d is %d generators wide: a state vector of width %d in HBM (%d at most) needs more than "
                                                         "the %d held generators a plan takes", code, L, tp.full_width, hbm_width, kTiledMaxWidth, kMaxHeld);
        return tp;
    }
    held.assign((size_t)p.n_gen, 0);
    while (p.width > hbm_width) {                                               // build_cut_plan's hold rule
        const int pick = pick_hold(tr, p.n_gen);
        if (pick < 0) { p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: no generator is live at the peak of code %d at L=%d", code, L); return tp; }
        if (tp.n_held == kMaxHeld) {
            p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "the frontier of code %d at L=%d is %d generators wide: %d held generators leave width %d, a state vector of width "
                                                             "%d in HBM (%d at most) needs more than that", code, L, tp.full_width, kMaxHeld, p.width, hbm_width, kTiledMaxWidth);
            return tp;
        }
        held[(size_t)pick] = 1; ++tp.n_held;
        st = build_stream(code, L, held, &tr);
        p = st.head;
        if (p.refusal.code) return tp;
    }
    if (st.live_at_end != 0) { p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: the plan of code %d at L=%d ends with %d live slots", code, L, st.live_at_end); return tp; }
    tp.state_bits = p.width > tile_width ? p.width : tile_width;
    // ---- the wide encoding
    for (const StreamOp &o : st.ops) {
        uint32_t mask = 0, top = 0, pair[4];
        for (size_t s = 0; s < o.live.size(); ++s)
            if (o.live[s]) mask |= 1u << s;
        const uint32_t reach = o.kind == kClose ? mask : mask | (1u << o.slot);
        while (top < 32u && (reach >> top)) ++top;
        if ((int)top > p.width || (int)o.qubit >= p.nq) { p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: an op of code %d at L=%d leaves its state vector", code, L); return tp; }
        for (int j = 0; j < 4; ++j) pair[j] = (uint32_t)j < o.pairs ? (o.pair_slot[j] & 31u) | (o.pair_xz[j] << 5) : 0u;
        tp.ops.push_back(o.kind | (o.slot << 4) | (o.pairs << 9) | (top << 12));
        tp.ops.push_back(mask);
        tp.ops.push_back(pair[0] | (pair[1] << 8) | (pair[2] << 16) | (pair[3] << 24));
        tp.ops.push_back(o.qubit);
    }
    // ---- the segments: the longest run whose INTRO / FORGET slots fit next to the low bits, from every segment's first op
    const uint32_t low = (1u << (tile_width > kTileLowBits ? kTileLowBits : tile_width - 1)) - 1u;
    for (int first = 0; first < p.n_ops;) {
        Segment sg;
        sg.op_first = (uint32_t)first; sg.tile = low;
        int o = first;
        for (; o < p.n_ops; ++o) {
            const uint32_t *op = &tp.ops[(size_t)o * kTiledOpWords];
            const uint32_t bit = (op[0] & 15u) == kClose ? 0u : 1u << ((op[0] >> 4) & 31u);
            if (!(sg.tile & bit) && bit && (int)popcount32(sg.tile) == tile_width) break;
            sg.tile |= bit;
        }
        sg.op_count = (uint32_t)(o - first);
        for (uint32_t b = 0; (int)popcount32(sg.tile) < tile_width; ++b) sg.tile |= 1u << b;          // (filled with the lowest bits it lacks: all below state_bits)
        sg.live_in = wide_before(&tp.ops[(size_t)first * kTiledOpWords]);
        sg.live_out = wide_after(&tp.ops[(size_t)(o - 1) * kTiledOpWords]);
        for (int i = first; i < o; ++i) {
            const uint32_t *op = &tp.ops[(size_t)i * kTiledOpWords];
            sg.live |= wide_before(op) | wide_after(op);
            if (((wide_before(op) ^ sg.live_in) | (wide_after(op) ^ sg.live_in)) & ~sg.tile) {
                p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: a segment of code %d at L=%d changes a slot outside its tile", code, L);
                return tp;
            }
        }
        sg.n_tiles = 1u << popcount32(sg.live & ~sg.tile);
        if (sg.op_count == 0 || (sg.tile >> tp.state_bits) != 0u) { p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: an empty segment of code %d at L=%d", code, L); return tp; }
        for (int i = first; i < o; ++i) {
            uint32_t d[kTiledDevOpWords];
            encode_dev_op(&tp.ops[(size_t)i * kTiledOpWords], sg.tile, d);
            tp.dev_ops.insert(tp.dev_ops.end(), d, d + kTiledDevOpWords);
        }
        tp.segments.push_back(sg);
        first = o;
    }
    if (tp.segments.empty() || tp.segments.front().live_in != 0u || tp.segments.back().live_out != 0u) {
        p.refusal = refuse_params(QECMC_ERR_UNSUPPORTED, "internal: the plan of code %d at L=%d does not start and end with an empty frontier", code, L);
        return tp;
    }
    finish_plan(p, st.table);
    held_generator_words(st.table, held, tp.held, tp.held_words);
    return tp;
}

// How a batch becomes launches.  Syndromes go in groups as the cut sweep's (their partials P[group][ncls][2^n_held] stay within kCutGridMax doubles);
// the (syndrome, class, assignment) units of a group go in passes whose state vectors fit kTiledWorkspaceBytes -- 2 048 units at width 16, 8 at 24.
inline uint32_t tiled_pass_units(int state_bits)
{
    const size_t fit = kTiledWorkspaceBytes >> (state_bits + 3);
    return fit < 1 ? 1u : fit > kTiledUnitsMax ? kTiledUnitsMax : (uint32_t)fit;
}
// threads of a workgroup: the kernel strides by blockDim.x, so the entries see the same operations whatever the number of lanes
constexpr uint32_t tiled_threads(int tile_width) { return tile_width >= 13 ? 1024u : tile_width <= 9 ? 64u : 1u << (tile_width - 3); }    // 8 entries per lane

// the representative of assignment h: rep times the held generators whose bit is set in h (cut_representative's rule)
inline void tiled_representative(const TiledPlan &tp, const uint32_t *rep, uint32_t h, uint32_t *out)
{
    for (int w = 0; w < tp.plan.W; ++w) {
        uint32_t v = rep[w];
        for (int j = 0; j < tp.n_held; ++j)
            if ((h >> j) & 1u) v ^= tp.held_words[(size_t)j * tp.plan.W + w];
        out[w] = v;
    }
}

// one representative through the wide stream, unscaled: sweep_one() entry for entry, walking the live indices only (the submasks of the op's mask)
inline double sweep_one_wide(const TiledPlan &tp, const uint32_t *rep, const double *wxz, double *A)
{
    A[0] = 1.0;
    host_ops_wide(tp.ops.data(), tp.plan.n_ops, rep, A, [&](double a, uint32_t, uint32_t idx) { return a * wxz[idx]; }, [](double a, double b) { return a + b; });
    return A[0];
}

// The twin.  chains uint8[N][nq], w[4] (I, X, Y, Z) -> Z double[N][ncls]; cls int32[N] (nullable).  The (class, assignment) units of one syndrome are
// spread over host threads (0: as many as the machine has, 16 at most, and no more than keep their state vectors within kTiledWorkspaceBytes); every
// partial and every sum is formed in the same order whatever their number.
inline void sweep_tiled_host(const TiledPlan &tp, uint64_t N, const uint8_t *chains, const double *w, double *Z, int32_t *cls, unsigned threads = 0)
{
    const Plan &p = tp.plan;
    double wxz[4];
    weights_xz(w, wxz);
    const uint32_t n_h = 1u << tp.n_held, n_work = (uint32_t)p.ncls * n_h;
    threads = host_threads(threads, n_work, tiled_pass_units(p.width), p.width < 12);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    std::vector<double> P((size_t)n_work);
    for (uint64_t s = 0; s < N; ++s) {
        const int a = class_representatives(p, chains + s * (uint64_t)p.nq, reps.data());
        if (cls) cls[s] = a;
        host_partials(n_work, threads, p.width, p.W, P.data(), [&](uint32_t i, uint32_t *rep, double *A) {
            tiled_representative(tp, &reps[(size_t)(i >> tp.n_held) * p.W], i & (n_h - 1u), rep);
            return sweep_one_wide(tp, rep, wxz, A);
        });
        for (int c = 0; c < p.ncls; ++c) Z[s * (uint64_t)p.ncls + c] = cut_reduce(&P[(size_t)c << tp.n_held], tp.n_held, p.scale);
    }
}

}  // namespace sweep

// class_sweep_tiled.hip: all pointers are device pointers.  dev_ops uint32[n_ops][kTiledDevOpWords]; held uint32[n_held][W]; reps uint32[S][ncls][W];
// work double[units][2^state_bits]: the state vectors of one pass, dirty; P double[S][ncls][2^n_held]: every entry written before it is read.
struct SweepTiledArgs {
    uint32_t unit_first, units;        // the units ((syndrome * ncls + class) << n_held) + h of this pass
    int W, n_held, state_bits, tile_width;
    uint32_t op_first, op_count;       // the segment
    uint32_t tile, fixed_live;         // T, and the occupied slots outside it: live & ~T
    uint32_t local_in, local_out;      // live_in and live_out within T, as local bits
    uint32_t n_tiles, first, last;     // first: nothing is gathered, A[0] = 1; last: the one live entry goes to P
    double wxz[4];
};
hipError_t launch_class_sweep_tiled(const sweep::TiledPlan &tp, const double *wxz, uint32_t unit_first, uint32_t units, const uint32_t *dev_ops, const uint32_t *held,
                                    const uint32_t *reps, double *work, double *P, hipStream_t stream);

#ifdef __HIPCC__
namespace sweep {

// HeldRep, then the CLOSE's pairs on fixed slots (word 4): the tile's own bits decide them
struct TileRep {
    HeldRep rep;
    uint32_t base;
    __device__ __forceinline__ uint32_t operator()(const uint32_t *op, uint32_t q) const
    {
        const uint32_t fixed = op[4];
        uint32_t cq = rep(op, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pr = (fixed >> (8 * j)) & 0xFFu;
            cq ^= (0u - ((base >> (pr & 31u)) & 1u)) & (pr >> 5);
        }
        return cq;
    }
};

// One workgroup of a tiled kernel, tile blockIdx.x of unit a.unit_first + blockIdx.y: gather the entries live at the segment's first op into lds
// (the first segment sets A[0] = 1), run the segment's ops there, store the entries live after its last op (the last segment: P[unit]).  Args is
// SweepTiledArgs or SweepTiledSiteArgs (or the (min, +) pair of class_minplus_tiled.hpp); src: the factors of a CLOSE.  Alg is the entry algebra and T
// its entry -- SumProduct over double, minplus::MinPlus over uint64_t --, T(1) the entry of the empty frontier: 1.0, or (cost 0, count 1).
// The gather and the write-back are restated, around a FORGET of their own, by minplus::tile_sweep_traced (class_minplus_tiled_trace.hpp) and by
// tile_sweep_recorded (class_sample_tiled.hip): a change to either loop here goes to both copies.
template <class Alg, class T, class Args, class Src>
__device__ __forceinline__ void tile_sweep(T *lds, const Args &a, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ held,
                                           const uint32_t *__restrict__ reps, T *__restrict__ work, T *__restrict__ P, const Src &src)
{
    static_assert(sizeof(T) == sizeof(double), "an entry is one 64-bit word: the workspace, tiled_pass_units and lds_carve are shared");
    const uint32_t tid = threadIdx.x, threads = blockDim.x, unit = a.unit_first + blockIdx.y, hbits = unit & ((1u << a.n_held) - 1u);
    const uint32_t base = bits_deposit(blockIdx.x, a.fixed_live), entries = 1u << a.tile_width;
    T *A = work + ((size_t)blockIdx.y << a.state_bits) + base;
    // local index l <-> offset f = l spread over T; the next one of a lane is `threads` further: an addition that carries across the bits outside T
    const uint32_t f0 = bits_deposit(tid, a.tile), step = bits_deposit(threads, a.tile);
    if (a.first) {
        if (tid == 0) lds[0] = T(1);
    } else {
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_in)) lds[l] = A[f];
    }
    __syncthreads();
    op_loop<TileOps, Alg>(lds, ops, a.op_first, a.op_count, tid, threads,
                          TileRep{HeldRep{reps + (size_t)(unit >> a.n_held) * (size_t)a.W, held, hbits, (uint32_t)a.W}, base}, src);
    if (a.last) {
        if (tid == 0) P[unit] = lds[0];
    } else {
        for (uint32_t l = tid, f = f0; l < entries; l += threads, f = ((f | ~a.tile) + step) & a.tile)
            if (!(l & ~a.local_out)) A[f] = lds[l];
    }
}

// The launches of one pass: one per segment of the plan, in order, on one stream.  `a` arrives with what is the caller's own; launch(a, segment)
// starts the kernel.  hipErrorInvalidValue for a plan or a pass the kernels do not take.
template <class Args, class Launch>
inline hipError_t tiled_segments(const TiledPlan &tp, uint32_t unit_first, uint32_t units, Args a, Launch launch)
{
    const Plan &p = tp.plan;
    if ((p.ncls != 4 && p.ncls != 16) || tp.tile_width < kTileMinWidth || tp.tile_width > kTileMaxWidth || tp.state_bits < tp.tile_width ||
        tp.state_bits > kTiledMaxWidth || p.W < 1 || p.n_ops < 1 || tp.n_held < 0 || tp.n_held > kMaxHeld || units > tiled_pass_units(tp.state_bits) ||
        tp.segments.empty())
        return hipErrorInvalidValue;
    a.unit_first = unit_first; a.units = units; a.W = p.W; a.n_held = tp.n_held; a.state_bits = tp.state_bits; a.tile_width = tp.tile_width;
    for (size_t s = 0; s < tp.segments.size(); ++s) {
        const Segment &sg = tp.segments[s];
        a.op_first = sg.op_first; a.op_count = sg.op_count; a.tile = sg.tile; a.fixed_live = sg.live & ~sg.tile;
        a.local_in = bits_extract(sg.live_in, sg.tile); a.local_out = bits_extract(sg.live_out, sg.tile);
        a.n_tiles = sg.n_tiles; a.first = s == 0; a.last = s + 1 == tp.segments.size();
        if ((int)popcount32(sg.tile) != tp.tile_width || (sg.tile >> tp.state_bits) != 0u || (sg.live >> tp.state_bits) != 0u ||
            sg.n_tiles != 1u << popcount32(a.fixed_live) || sg.op_first + sg.op_count > (uint32_t)p.n_ops)
            return hipErrorInvalidValue;
        launch(a, sg);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace sweep
#endif  // __HIPCC__

}  // namespace qecmc
