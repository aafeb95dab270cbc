// qecmc_coset_enumerate: the histogram H[c][n_xy][n_z] of enumerate.hpp over one chunk of the stabilizer group, for a group of syndromes.
//
// Workgroup (blockIdx.x, blockIdx.y) works on syndrome blockIdx.y and on elements [blockIdx.x << slice_bits, +2^slice_bits) of the chunk.  A thread takes
// a base index that is a multiple of 2^T, forms its start planes from the basis generators set in the base (bits T .. chunk_bits - 1: the table rows are
// addressed by the loop counter alone -- scalar loads -- and a lane's bit only selects) and walks the span of the low T generators by the ruler sequence
// ctz(i): unrolled over the compile-time T, so which generator a step XORs is a constant, the same in every lane, and its planes stay in scalar
// registers -- as the representatives of the NCLS classes do, with the chunk's own product folded in.  Per element and class: two XORs, two population
// counts, one LDS add into the lane's copy of the histogram (32-bit counters: a workgroup adds at most 2^slice_bits <= 2^30 to one).  The
// non-zero bins are flushed to the uint64 output with integer atomics: exact and order-independent.  Nothing here grows with the rank or with N.
#include "enumerate.hpp"

namespace qecmc {

template <int NCLS, int T>
__global__ __launch_bounds__(enumr::kThreads) void k_enumerate(const EnumArgs a, const uint32_t *__restrict__ gen, const uint32_t *__restrict__ reps,
                                                               unsigned long long *__restrict__ hist)
{
    extern __shared__ uint32_t enum_lds[];                    // [copies][NCLS][bins]
    const uint32_t tid = threadIdx.x, copy_words = (uint32_t)NCLS * a.bins;
    for (uint32_t i = tid; i < a.copies * copy_words; i += enumr::kThreads) enum_lds[i] = 0u;
    __syncthreads();
    // byte offsets of this lane's copy of the NCLS histograms and of a row of one.  Neighbouring lanes add into different copies: the adds of one wave
    // instruction that meet in a bin serialise, and the counts of a wavefront's 64 elements cluster in a few bins (measured: 1.6 - 2.1 times the rate
    // of one copy per wavefront, at the same instruction count)
    const uint32_t mine = (tid % a.copies) * copy_words * 4u, row_bytes = a.nq1 * 4u;
    uint32_t rx[NCLS], rz[NCLS], lx[T], lz[T];
    const uint32_t *rep = reps + (size_t)blockIdx.y * (size_t)(2 * NCLS);
#pragma unroll
    for (int c = 0; c < NCLS; ++c) { rx[c] = rep[2 * c] ^ a.cx; rz[c] = rep[2 * c + 1] ^ a.cz; }
#pragma unroll
    for (int j = 0; j < T; ++j) { lx[j] = gen[2 * j]; lz[j] = gen[2 * j + 1]; }
    const uint32_t chunk_elems = 1u << a.chunk_bits, slice_first = blockIdx.x << a.slice_bits;
    const uint32_t passes = 1u << (a.slice_bits - T - 8);
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t base = slice_first + ((pass * enumr::kThreads + tid) << T);
        if (base >= chunk_elems) continue;                    // (a chunk shorter than one pass of the workgroup)
        uint32_t x = 0u, z = 0u;
        for (int b = T; b < a.chunk_bits; ++b) {
            const uint32_t on = 0u - ((base >> b) & 1u);
            x ^= gen[2 * b] & on; z ^= gen[2 * b + 1] & on;
        }
#pragma unroll
        for (int i = 0; i < (1 << T); ++i) {
            if (i) { x ^= lx[__builtin_ctz(i)]; z ^= lz[__builtin_ctz(i)]; }
#pragma unroll
            for (int c = 0; c < NCLS; ++c) {
                const uint32_t xx = x ^ rx[c], zz = z ^ rz[c];
                const uint32_t row = __umul24((uint32_t)__popc(xx), row_bytes) + (mine + (uint32_t)c * a.bins * 4u);
                atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(enum_lds) + (((uint32_t)__popc(zz & ~xx) << 2) + row)), 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long *out = hist + (size_t)blockIdx.y * (size_t)copy_words;
    for (uint32_t i = tid; i < copy_words; i += enumr::kThreads) {
        unsigned long long sum = 0ull;
        for (uint32_t k = 0; k < a.copies; ++k) sum += enum_lds[k * copy_words + i];
        if (sum) atomicAdd(&out[i], sum);
    }
}

hipError_t launch_enumerate(const EnumArgs &a, const uint32_t *gen, const uint32_t *reps, unsigned long long *hist, hipStream_t stream)
{
    if (a.S == 0) return hipSuccess;
    const int T = enumr::walk_bits(a.ncls);
    const size_t lds = (size_t)a.copies * (size_t)a.ncls * a.bins * sizeof(uint32_t);
    if ((a.ncls != 4 && a.ncls != 16) || a.copies == 0 || lds > enumr::kLdsBudget || a.nq1 * a.nq1 != a.bins || a.nq1 > (uint32_t)enumr::kMaxQubits + 1u ||
        a.chunk_bits < enumr::kMinChunkBits || a.chunk_bits > enumr::kMaxChunkBits || a.slice_bits < T + 8 || a.slice_bits > enumr::kMaxChunkBits ||
        a.S > 65535u || a.blocks == 0 || ((uint64_t)a.blocks << a.slice_bits) > (1ull << enumr::kMaxChunkBits))
        return hipErrorInvalidValue;
    const dim3 grid(a.blocks, a.S), block(enumr::kThreads);
    if (a.ncls == 16) hipLaunchKernelGGL((k_enumerate<16, enumr::walk_bits(16)>), grid, block, lds, stream, a, gen, reps, hist);
    else hipLaunchKernelGGL((k_enumerate<4, enumr::walk_bits(4)>), grid, block, lds, stream, a, gen, reps, hist);
    return hipGetLastError();
}

}  // namespace qecmc
