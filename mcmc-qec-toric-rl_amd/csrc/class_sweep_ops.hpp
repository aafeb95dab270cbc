// The op loop of the class sweeps -- INTRO / CLOSE / FORGET over a state vector A[2^width] -- written once for the device and once, apart, for the
// host.  class_sweep.hpp describes the stream and the plan; every kernel of the family (class_sweep*.hip, class_minplus*.hip) and every host twin
// (sweep_one*, minplus_one*) runs the loops below with its own entry algebra and its own source of a CLOSE's factors.
//
// THE DEVICE LOOP (op_loop).  The state vector is in LDS and is updated in place.  The plan is the same for every workgroup and is addressed by the
// loop counter alone, the representative's packed words by the block index and the op's qubit, the held words by the block's assignment: scalar
// loads, wave-uniform control flow.  An op walks the indices below its `top` -- the ranges above the highest occupied slot are skipped -- and leaves
// out an index with a bit outside its mask: only live entries are read, and every live entry was written by the INTRO that made it live, so dirty
// LDS does not matter (A[0] is the one word a kernel sets up).  One barrier after every op.  INTRO and FORGET walk the half index h with a zero
// inserted at the slot: consecutive lanes touch consecutive 8-byte entries in runs of 2^slot, so slots below 4 read two 256-byte bank rows per
// 32-lane group (2-way) and the others one; CLOSE is unit stride.  A CLOSE's factors are fetched once, outside the per-entry loop, under
// wave-uniform control flow.  Every entry sees exactly the operation sequence of the host loop: copies, one `close` and one `forget` at a time --
// single multiplies and single adds for the sum-product, an add to the cost field and mp_combine for (min, +).  Nothing here grows with N.
//
// THE HOST LOOPS (host_ops, host_ops_wide) are written independently of the device loop and share no loop body with it: that a twin written apart
// agrees with its kernel bit for bit is the project's correctness argument, and one __host__ __device__ body for both would make every parity test
// vacuous.  Shared between the two sides is only what always was: insert_zero, pauli_to_xz, and the entry helpers of the other headers (site_cost,
// mp_combine, mp_unpack, remove_bit).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

namespace qecmc {
namespace sweep {

// One op of the narrow stream is four words:
//     [0]  kind | slot << 4 | pairs << 8 | top << 12     top: the index bits the op walks -- every bit of mask, and the op's own slot, lies below it
//     [1]  mask      the occupied slots: INTRO before it, CLOSE as they are, FORGET after it
//     [2]  CLOSE: four bytes (slot | xz << 4), xz = x | z << 1 of the generator's Pauli at the qubit; bytes beyond `pairs` are 0 (they change nothing)
//     [3]  CLOSE: the qubit
// The wide stream (class_sweep_tiled.hpp) keeps a slot in 5 bits, and its device form has a fifth word and `top` at bit 8.
constexpr uint32_t kIntro = 0, kClose = 1, kForget = 2;
constexpr int kOpWords = 4;
struct NarrowOps { static constexpr uint32_t kWords = 4, kTopShift = 12; };   // build_plan_held()'s encoding
struct TileOps { static constexpr uint32_t kWords = 5, kTopShift = 8; };      // encode_dev_op()'s

__host__ __device__ inline uint32_t pauli_to_xz(uint32_t p) { return (p ^ (p >> 1)) & 3u; }      // I X Y Z = 0 1 2 3 -> 0 1 3 2 (and back)

// the index with a zero inserted at bit `slot` of h
__host__ __device__ inline uint32_t insert_zero(uint32_t h, uint32_t slot) { return ((h >> slot) << (slot + 1u)) | (h & ((1u << slot) - 1u)); }

// ---------------------------------------------------------------- the host loops
// FORGETs that keep nothing; minplus::Decisions (class_minplus_trace.hpp) keeps which branch won
struct NoDecisions {
    void begin(uint32_t) {}
    template <class T> void at(uint32_t, T, T) {}
    void end() {}
};

// The narrow stream over A, A[0] set by the caller.  close(a, q, idx): the entry after the CLOSE of qubit q at idx = x | z << 1; forget(a, b): the
// entry after a FORGET.  At a FORGET, decide.begin(2^(top - 1)) comes first, decide.at(h, A[f], A[f | bit]) before every live entry is combined,
// decide.end() last.
template <class T, class Close, class Forget, class Decide>
inline void host_ops(const uint32_t *ops, int n_ops, const uint32_t *rep, T *A, Close close, Forget forget, Decide &&decide)
{
    for (int o = 0; o < n_ops; ++o) {
        const uint32_t *op = ops + (size_t)o * kOpWords;
        const uint32_t kind = op[0] & 15u, slot = (op[0] >> 4) & 15u, top = (op[0] >> 12) & 31u, mask = op[1], bit = 1u << slot;
        if (kind == kClose) {
            const uint32_t q = op[3], cq = pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
            for (uint32_t f = 0; f < (1u << top); ++f) {
                if (f & ~mask) continue;
                uint32_t idx = cq;
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (op[2] >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                }
                A[f] = close(A[f], q, idx);
            }
            continue;
        }
        const uint32_t n_h = 1u << (top - 1u);
        if (kind == kForget) decide.begin(n_h);
        for (uint32_t h = 0; h < n_h; ++h) {
            const uint32_t f = insert_zero(h, slot);
            if (f & ~mask) continue;
            if (kind == kIntro) { A[f | bit] = A[f]; continue; }
            decide.at(h, A[f], A[f | bit]);
            A[f] = forget(A[f], A[f | bit]);
        }
        if (kind == kForget) decide.end();
    }
}

// The wide stream (four words, slots in 5 bits) over A, walking the live indices only: the submasks of the op's mask
template <class T, class Close, class Forget> inline void host_ops_wide(const uint32_t *ops, int n_ops, const uint32_t *rep, T *A, Close close, Forget forget)
{
    for (int o = 0; o < n_ops; ++o) {
        const uint32_t *op = ops + (size_t)o * 4u;
        const uint32_t kind = op[0] & 15u, bit = 1u << ((op[0] >> 4) & 31u), mask = op[1];
        uint32_t f = 0;
        if (kind == kClose) {
            const uint32_t q = op[3], cq = pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
            do {
                uint32_t idx = cq;
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pr = (op[2] >> (8 * j)) & 0xFFu;
                    idx ^= (0u - ((f >> (pr & 31u)) & 1u)) & (pr >> 5);
                }
                A[f] = close(A[f], q, idx);
                f = (f - mask) & mask;
            } while (f);
        } else if (kind == kIntro) {
            do { A[f | bit] = A[f]; f = (f - mask) & mask; } while (f);
        } else {
            do { A[f] = forget(A[f], A[f | bit]); f = (f - mask) & mask; } while (f);
        }
    }
}

// threads of a twin that spreads `n_work` partials over host threads: 0 is as many as the machine has; 16 at most, `cap` at most, one per partial
// at most, and one where `serial`
inline unsigned host_threads(unsigned threads, uint32_t n_work, uint32_t cap, bool serial)
{
    if (threads == 0) threads = std::thread::hardware_concurrency();
    if (threads > 16u) threads = 16u;
    if (threads > cap) threads = cap;
    if (threads > n_work) threads = n_work;
    return threads < 1u || serial ? 1u : threads;
}

// the partials P[n_work] of one syndrome over `threads` host threads, each formed alone by one(i, rep scratch [W], A scratch [2^width]): the result
// does not depend on their number
template <class T, class One> inline void host_partials(uint32_t n_work, unsigned threads, int width, int W, T *P, One one)
{
    auto work = [&](unsigned t) {
        std::vector<T> A((size_t)1 << width);
        std::vector<uint32_t> rep((size_t)W);
        for (uint32_t i = t; i < n_work; i += threads) P[i] = one(i, rep.data(), A.data());
    };
    if (threads <= 1u) { threads = 1u; work(0); return; }
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t) pool.emplace_back(work, t);
    for (std::thread &t : pool) t.join();
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- the device loop
// A CLOSE's four factors, fetched once per CLOSE; at(idx) picks with two selects
template <class V> struct Four {
    V v00, v01, v10, v11;
    __device__ __forceinline__ V at(uint32_t idx) const
    {
        const V lo = (idx & 1u) ? v01 : v00, hi = (idx & 1u) ? v11 : v10;
        return (idx & 2u) ? hi : lo;
    }
};
// ... the same four for every qubit (kernel arguments), or the row of qubit q in a table of four per qubit (wave-uniform scalar loads)
template <class V> struct UniformFour {
    const V *v;
    __device__ __forceinline__ Four<V> row(uint32_t) const { return {v[0], v[1], v[2], v[3]}; }
};
template <class V> struct SiteFour {
    const V *rows;
    __device__ __forceinline__ Four<V> row(uint32_t q) const
    {
        const V *w = rows + (size_t)q * 4u;
        return {w[0], w[1], w[2], w[3]};
    }
};

// the (x, z) of the qubit's Pauli in the representative: its packed word, XOR the same word of every held generator whose bit is set in hbits
struct Rep {
    const uint32_t *rep;
    __device__ __forceinline__ uint32_t operator()(const uint32_t *, uint32_t q) const { return pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u); }
};
struct HeldRep {
    const uint32_t *rep, *held;
    uint32_t hbits, W;
    __device__ __forceinline__ uint32_t operator()(const uint32_t *, uint32_t q) const
    {
        uint32_t word = rep[q >> 4];
        for (uint32_t rest = hbits; rest; rest &= rest - 1u) word ^= held[(uint32_t)(__ffs(rest) - 1) * W + (q >> 4)];
        return pauli_to_xz((word >> ((q & 15u) * 2u)) & 3u);
    }
};

// the sum-product: doubles, one multiply at a CLOSE, one add at a FORGET
struct SumProduct {
    static __device__ __forceinline__ double close(double a, double w) { return a * w; }
    static __device__ __forceinline__ double forget(double a, double b) { return a + b; }
};

// an op's words, decoded: Fmt names the stride and where `top` sits
template <class Fmt> struct Op {
    const uint32_t *w;
    uint32_t kind, slot, top, mask;
    __device__ __forceinline__ Op(const uint32_t *ops, uint32_t o) : w(ops + Fmt::kWords * o)
    {
        const uint32_t w0 = w[0];
        mask = w[1];
        kind = w0 & 15u; slot = (w0 >> 4) & 15u; top = (w0 >> Fmt::kTopShift) & 31u;
    }
};

// CLOSE: the (x, z) index of every live entry -- the qubit's own, folded with the pairs whose slot bit is set in f -- picks the factor
template <class Alg, class Fmt, class T, class RepXz, class Src>
__device__ __forceinline__ void close_pass(T *A, uint32_t tid, uint32_t threads, const Op<Fmt> &op, const RepXz &rep, const Src &src)
{
    const uint32_t pairs = op.w[2], q = op.w[3];
    const uint32_t cq = rep(op.w, q);
    const auto row = src.row(q);
    for (uint32_t f = tid; f < (1u << op.top); f += threads) {
        if (f & ~op.mask) continue;
        uint32_t idx = cq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pr = (pairs >> (8 * j)) & 0xFFu;
            idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
        }
        A[f] = Alg::close(A[f], row.at(idx));
    }
}

// INTRO and FORGET: one walk over the half index, the kind tested per entry under a wave-uniform branch -- the one loop the sweep kernels have always
// had; splitting it doubles the index code (15 vector instructions and an LDS read more).  A caller that knows the kind leaves one of the two behind.
template <class Alg, class Fmt, class T> __device__ __forceinline__ void half_pass(T *A, uint32_t tid, uint32_t threads, const Op<Fmt> &op, uint32_t kind)
{
    const uint32_t bit = 1u << op.slot;
    for (uint32_t h = tid; h < (1u << (op.top - 1u)); h += threads) {
        const uint32_t f = insert_zero(h, op.slot);
        if (f & ~op.mask) continue;
        if (kind == kIntro) A[f | bit] = A[f];
        else A[f] = Alg::forget(A[f], A[f | bit]);
    }
}
template <class Alg, class Fmt, class T> __device__ __forceinline__ void intro_pass(T *A, uint32_t tid, uint32_t threads, const Op<Fmt> &op)
{
    half_pass<Alg>(A, tid, threads, op, kIntro);
}

// Ops [first, first + count) of a stream in format Fmt over A, one barrier per op.  rep(op words, q): the (x, z) the CLOSE of qubit q starts from;
// src.row(q): its factors.
template <class Fmt, class Alg, class T, class RepXz, class Src>
__device__ __forceinline__ void op_loop(T *A, const uint32_t *__restrict__ ops, uint32_t first, uint32_t count, uint32_t tid, uint32_t threads, const RepXz &rep,
                                        const Src &src)
{
    for (uint32_t o = first; o < first + count; ++o) {
        const Op<Fmt> op(ops, o);
        if (op.kind == kClose) close_pass<Alg>(A, tid, threads, op, rep, src);
        else half_pass<Alg>(A, tid, threads, op, op.kind);
        __syncthreads();
    }
}
#endif  // __HIPCC__

}  // namespace sweep
}  // namespace qecmc
