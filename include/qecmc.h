/*
 * qecmc.h -- C-ABI of the MI355X-native MCMC equivalence-class sampler.
 *
 * This is the drop-in boundary for ONE hot path of
 * QEC-project-2020/MCMC-QEC-toric-RL: the Metropolis / parallel-tempering
 * sampler of src/mcmc.py, the code-model stencils it calls
 * (src/toric_model.py ...) and its caller decoders.PTEQ.  The reference has no
 * FFI of its own (it is pure Python + numba); the boundary below is what a
 * `ctypes.CDLL` binding on the reference side would load (INTEGRATION.md shows
 * that binding).  Every entry point cites the reference interface it replaces
 * (file:line relative to the reference tree).
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer and the
 *     library keeps no pointer after a call returns (plans excepted);
 *   - return 0 on success, a negative qecmc_status on error with a message in
 *     qecmc_last_error() (thread-local); no C++ exception crosses the ABI;
 *   - Pauli encoding 0=I 1=X 2=Y 3=Z, composition = XOR (toric_model.py:277);
 *     toric state = uint8[2][L][L] C-order (toric_model.py:12), nq = 2*L*L; xzzx / rotated state = uint8[L][L];
 *     planar state = uint8[2][L][L] with layer 1 on its first L-1 rows / columns (planar_model.py:14,38-39);
 *   - every compute entry point runs on the GPU (HIP, gfx950).  There is no
 *     CPU fallback: without a device the call fails with QECMC_ERR_NO_DEVICE.
 *   - `_dev` entry points take DEVICE pointers and a hipStream_t (as void*),
 *     enqueue asynchronously and allocate nothing; the others take HOST
 *     pointers and do H2D + kernel + D2H + synchronise themselves.
 */
#ifndef QECMC_H
#define QECMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QECMC_ABI_VERSION 4

typedef enum qecmc_status {
    QECMC_OK = 0,
    QECMC_ERR_INVALID = -1,     /* bad argument (message says which) */
    QECMC_ERR_NO_DEVICE = -2,   /* no HIP device / device index out of range */
    QECMC_ERR_HIP = -3,         /* a HIP runtime call failed */
    QECMC_ERR_UNSUPPORTED = -4  /* valid request this build has no kernel for */
} qecmc_status;

typedef enum qecmc_code { QECMC_TORIC = 0, QECMC_XZZX = 1, QECMC_ROTATED = 2, QECMC_PLANAR = 3 } qecmc_code;
/* SWEEP: systematic sweep over the generators in table order (proposal k tests generator k mod G); no colouring is needed
 * because a lane owns a whole chain.  Same stationary law, not the reference's chain. */
/* COLOUR: the latency layout -- one workgroup per ladder, one wavefront per rung, the lanes of a wavefront = the generators of
 * one colour phase (mutually disjoint, so their Metropolis tests are independent), proposed at once: a sweep is n_phases wavefront
 * passes instead of G sequential proposals.  A systematic scan like SWEEP (same stationary law, not the reference's chain);
 * `iters` counts phases; fixed-length runs report the first step with tops0 >= TOPS in steps_done / converged,
 * conv_mode error_based runs the reference's criterion.  Under the biased and alpha rules (xzzx / rotated codes) every
 * generator is a Metropolis move for the noise model's own weight px^nx py^ny pz^nz pI^nI -- the reference's rule at iters = 1: the members
 * of a phase are tested at once, so the p_b that mcmc_biased.py:28-31 / mcmc_alpha.py:38-41 freeze per update_chain call cannot be
 * carried --; the biased top rung tests its logical operators, Ladder_alpha's top rung (pz_tilde = 1) takes the coin. */
/* WAVE: the reference's random scan (src/mcmc.py:19-43) with ONE generator pick per proposal shared by the 64 ladders of a wavefront
 * (global ladder indices that agree above bit 6), every ladder keeping its own acceptance uniform.  toric_model.py:287-296 picks the
 * generator independently of the state and syndromes never interact, so each ladder's chain has exactly the reference's law -- unlike
 * SWEEP / COLOUR this IS the reference's Markov chain per syndrome; only the noise of different syndromes is correlated.  What it buys:
 * a proposal's sites are wave-uniform, so the rungs' states live in registers.  Depolarizing rule with a top rung at
 * p = 0.75 (Nc >= 2), at most 16 packed state words per rung (toric / planar L <= 11, xzzx / rotated L <= 16) -- fixed-length runs of
 * up to 8 rungs also 17 .. 32 words (toric L <= 16, xzzx / rotated L <= 22) --, and the alpha rule (xzzx / rotated L <= 11);
 * first_syndrome a multiple of 64, 1 <= iters <= 128.  With conv_mode error_based the launch runs on a persistent grid
 * whose workgroups own contiguous shares of the batch and reuse the lane of a stopped ladder for the next one of their share: the
 * generator picks then belong to the lane's position in the grid, so results are reproducible for a given (batch size, grid,
 * first_syndrome) and equal to the one-ladder-per-lane layout whenever the batch fits the grid; no final states in that mode.
 * Range of p (depolarizing rule): RANDOM and WAVE serve (0, 0.75] -- WAVE below the p at which a swap threshold leaves 32 bits (rungs that
 * coincide at p = 0.75 or nearly, p_diff > 1 - 2^-32) --; SWEEP and COLOUR are refused (QECMC_ERR_UNSUPPORTED) where ((p / 3) / (1 - p))^4
 * underflows to 0 in double precision, below p = 3.76e-81: every p >= 1e-80 is served ("Range"). */
typedef enum qecmc_scan { QECMC_SCAN_RANDOM = 0, QECMC_SCAN_SWEEP = 1, QECMC_SCAN_COLOUR = 2, QECMC_SCAN_WAVE = 3 } qecmc_scan;
typedef enum qecmc_noise { QECMC_NOISE_DEPOLARIZING = 0, QECMC_NOISE_BIASED = 1, QECMC_NOISE_ALPHA = 2 } qecmc_noise;
typedef enum qecmc_conv { QECMC_CONV_NONE = 0, QECMC_CONV_ERROR_BASED = 1 } qecmc_conv;

/* Mirrors the keyword arguments of decoders.PTEQ (decoders.py:25) plus what the
 * batched GPU call needs.  Set abi_size = sizeof(qecmc_params). */
typedef struct qecmc_params {
    uint32_t abi_size;
    int32_t  code;          /* qecmc_code */
    int32_t  L;             /* system_size (toric_model.py:10).  The ladder calls keep every rung's state, the generator table and the
                               acceptance tables in one workgroup's LDS, and refuse (QECMC_ERR_UNSUPPORTED, with the numbers) what does not fit:
                               Nc * ceil(nq / 16) * 256 B of states + tables <= 160 KiB (toric L = 20 at Nc = 8, L = 31 at Nc = 2), at most 2048
                               generators (toric L <= 32, xzzx / rotated L <= 45), nq <= 511 for the biased / alpha rules (L <= 21) */
    int32_t  Nc;            /* number of chains in the ladder (decoders.py:30; Q7: default L) */
    int32_t  noise;         /* qecmc_noise */
    int32_t  scan;          /* qecmc_scan: RANDOM = the reference's chain (src/mcmc.py:19-43) */
    int32_t  conv_mode;     /* qecmc_conv (decoders.py:74) */
    int32_t  device;        /* HIP device ordinal */
    uint64_t iters;         /* proposals per chain between swap sweeps (decoders.py:25 iters=10) */
    uint64_t steps;         /* ladder steps (decoders.py:25 steps) */
    int32_t  tops_burn;     /* decoders.py:63 */
    int32_t  TOPS;          /* decoders.py:74 */
    int32_t  SEQ;           /* decoders.py:78 */
    int32_t  replicas;      /* 0 or 1: one ladder per syndrome.  R > 1: R independent ladders per syndrome (Philox syndrome
                               index first_syndrome + s*R + r), class counts / samples / tops0 summed over the R ladders on the
                               device -- the reference's "droplets" pattern (decoders.py:215-225) for small batches */
    double   eps;           /* decoders.py:102 */
    double   p;             /* bottom-chain error rate (mcmc.py:50 p_bottom); pz_tilde_bottom for alpha noise (mcmc_alpha.py:76) */
    double   eta;           /* bias (mcmc_biased.py:11); unused otherwise */
    double   alpha;         /* alpha noise exponent (mcmc_alpha.py:11, decoders_biasednoise.py:175); unused otherwise */
    double   p_logical;     /* top-chain logical proposal rate (decoders.py:52 passes 0.5); the ladder kernels' random scan selects with
                               16 bits, i.e. acts as ceil(p_logical * 2^16) / 2^16 (exact for 0.5; the CPU oracle does the same) */
    uint64_t seed;          /* Philox key */
    uint32_t first_syndrome;/* global index of syndrome 0 of this call: results do not
                               depend on how a batch is sharded over GPUs */
    uint32_t flags;         /* 0 in production.  Developer switches (results are identical with any value; they select among kernel
                               variants that compute the same thing): QECMC_FLAG_* below in bits 0-15, and in bits 16-31 the size of
                               the work-queue kernels' persistent grid in workgroups (0: what fits the chip; the tests force 1-2
                               workgroups so that every lane runs several ladders) */
} qecmc_params;

enum qecmc_flag {
    QECMC_FLAG_NO_PRE   = 2,   /* no instantiations that draw the top chain's Philox blocks ahead */
    QECMC_FLAG_NO_DELUT = 4,   /* no dE look-up table (popcount form) */
    QECMC_FLAG_NO_SSW   = 8,   /* no swap sweep run once per workgroup (every wave replays the cascade): ladder_kernel's variant run by wave 0, and
                                  the scan = wave kernels' cascade walked by the top rung's wave (5 - 8 rungs, fixed length, up to 16 words) */
    QECMC_FLAG_NO_SPREAD = 16  /* the scan = wave kernels' walked cascade with every swap bound found by the top rung's wave, not a pair per wave below it */
};
#define QECMC_FLAGS_QUEUE_GRID(n) ((uint32_t)(n) << 16)

typedef struct qecmc_stats {
    uint64_t proposals;     /* Metropolis trials executed (all chains, all syndromes) */
    uint64_t swap_tests;
    double   kernel_ms;     /* HIP-event time of the sampler kernel(s) */
    double   total_ms;      /* wall time incl. H2D/D2H for host-pointer calls */
} qecmc_stats;

int         qecmc_abi_version(void);
const char *qecmc_last_error(void);
/* The kernel the calling thread's last ladder launch ran (PTEQ, PTDC, Ladder.step, ... -- every entry point that runs a ladder kernel): ten numbers,
 * family (1 ladder_kernel, 2 the scan = wave kernels, 3 the scan = colour kernels), maxt (the launch bound in threads), minw (waves per SIMD), code,
 * flags (ladder_kernel: its variant mask; wave / colour: 0, 1 = the statistics kernels, 2 = the shortest-chain kernels), wv (state words per rung, wave),
 * conv, it (the unrolled iters, 0: the general loop), alpha, rule (colour).  tools/kernel_resources.py key_label() names it as the build's resource
 * tables do.  QECMC_ERR_INVALID while the thread has launched nothing; a call of N = 0 and a refused launch leave the answer as it was.  For tests and
 * tools: which kernel a shape runs is not part of the ABI's promises (additive: QECMC_ABI_VERSION stays). */
int         qecmc_last_kernel(int64_t key_out[10]);
int         qecmc_device_count(void);      /* 0 when no GPU is visible */

/* ---- stencil primitives (batched; N states per call, host pointers) -------
 * Each runs the same __device__ stencil code the sampler kernels use. */

/* Toric_code.apply_stabilizer -> _apply_stabilizer, toric_model.py:40-41,256-284 (xzzx_model.py:360-436,
 * rotated_surface_model.py:349-392: operator 1 = plaquette (row,col), 3 = half plaquette `row` on side `col`;
 * planar_model.py:292-339: operator 1 at (row < L-1, col < L), operator 3 at (row < L, col < L-1)).
 * out[i] = in[i] with stabilizer (rows[i], cols[i], ops[i]) applied; dE[i] = error-count change. */
int qecmc_apply_stabilizer(int code, int L, uint64_t N, const uint8_t *in, uint8_t *out,
                           const int32_t *rows, const int32_t *cols, const int32_t *ops, int32_t *dE);
/* _apply_logical, toric_model.py:179-225 (layer is ignored by non-toric codes). */
int qecmc_apply_logical(int code, int L, uint64_t N, const uint8_t *in, uint8_t *out,
                        const int32_t *ops, const int32_t *layers, const int32_t *xpos,
                        const int32_t *zpos, int32_t *dE);
/* Toric_code.count_errors -> _count_errors, toric_model.py:33-34,174-176. */
int qecmc_count_errors(int code, int L, uint64_t N, const uint8_t *in, int64_t *n);
/* define_equivalence_class, toric_model.py:52-53,317-351. */
int qecmc_eq_class(int code, int L, uint64_t N, const uint8_t *in, int32_t *cls);
/* to_class, toric_model.py:55-56,354-377. */
int qecmc_to_class(int code, int L, uint64_t N, const uint8_t *in, uint8_t *out, const int32_t *eq);
/* Toric_code.syndrom, toric_model.py:58-101: defects_out uint8[N][2][L][L]; xzzx_code.syndrome /
 * RotSurCode.syndrome (xzzx_model.py:60-83): defects_out uint8[N][L+1][L+1] (plaquette_defects); Planar_code.syndrom
 * (planar_model.py:134-153): defects_out uint8[N][2 L (L-1)] = vertex_defects [L-1][L] then plaquette_defects [L][L-1]. */
int qecmc_syndrome(int code, int L, uint64_t N, const uint8_t *in, uint8_t *defects_out);

/* ---- syndrome generation (the data-generation recipe of generate_data.py:57-60,110-131, batched) --------------------
 * N random error chains -- Toric_code.generate_random_error(p) (toric_model.py:15-23; pass p_x = p_y = p_z = p / 3) or
 * generate_random_error(p_x, p_y, p_z) of the xzzx / rotated / planar models (xzzx_model.py:16-30, planar_model.py:18-40) --
 * then, if hide_class != 0, one apply_random_logical on each (generate_data.py:131), all on the device.
 * init_out uint8[N][nq] = the seed configurations for the decoder; raw_out (nullable) = the errors themselves
 * (generate_data.py:120 keeps them); eq_true_out (nullable) int32[N] = their equivalence class (:121-122), the decoding target.
 * Syndrome s draws from Philox (seed, first_syndrome + s): independent of how a data set is cut into batches.
 * The _dev form takes device pointers and a hipStream_t, allocates nothing and does not synchronise. */
int qecmc_generate_syndromes(int code, int L, uint64_t N, double p_x, double p_y, double p_z, int hide_class,
                             uint64_t seed, uint32_t first_syndrome, uint8_t *init_out, uint8_t *raw_out,
                             int32_t *eq_true_out);
int qecmc_generate_syndromes_dev(int code, int L, uint64_t N, double p_x, double p_y, double p_z, int hide_class,
                                 uint64_t seed, uint32_t first_syndrome, void *d_init_out, void *d_raw_out,
                                 void *d_eq_true_out, void *hip_stream);

/* ---- start chains from bare syndromes (no counterpart in the reference, whose entry points all start from an error chain) ------
 * defects uint8[N][cells] in the layout qecmc_syndrome writes (a non-zero byte = a defect) -> chains_out uint8[N][nq], a Pauli
 * configuration with exactly that syndrome: what qecmc_pteq_batch takes as `init`.  chain = XOR, over the set cells, of the rows of
 * the code's lift table (one Pauli string per check whose syndrome is that check alone -- on the torus plus its component's root
 * check; built by breadth-first search over the single-qubit X / Z errors, csrc/syndrome_lift.hpp); descend != 0 then sweeps the
 * stabilizer generators in table order, applying one iff it lowers the error count, until a whole sweep applies nothing (at most
 * nq + 1 sweeps).  No matching: the chain is a local minimum of the weight, in an arbitrary equivalence class.
 * status_out uint8[N] (nullable): 0 lifted; 1 not a syndrome of this code (a set cell that is no check, or an odd number of defects in
 * a component without boundary) -- that chain is all zero.  weight_out int32[N] (nullable): count_errors of the chain, -1 with status 1.
 * Additive: QECMC_ABI_VERSION stays.  A NULL buffer or a (code, L) the library does not know is refused (QECMC_ERR_INVALID) before a
 * device is looked for.
 * qecmc_lift: the uploaded table of one (code, L), on the device current when it was created.  The _dev form takes device pointers and
 * a hipStream_t, allocates nothing and does not synchronise (it composes with qecmc_generate_syndromes_dev / qecmc_pteq_launch_dev);
 * the lift must outlive the launches enqueued with it. */
int qecmc_chains_from_syndromes(int code, int L, uint64_t N, const uint8_t *defects, int descend, uint8_t *chains_out,
                                uint8_t *status_out, int32_t *weight_out);
typedef struct qecmc_lift qecmc_lift;
int qecmc_lift_create(int code, int L, qecmc_lift **out);
int qecmc_lift_destroy(qecmc_lift *lift);
int qecmc_chains_from_syndromes_dev(qecmc_lift *lift, const void *d_defects, uint64_t N, int descend, void *d_chains_out,
                                    void *d_status_out /*nullable*/, void *d_weight_out /*nullable*/, void *hip_stream);

/* ---- corrections from decoded syndromes (no counterpart in the reference, which returns a class histogram) -----------------------
 * candidates uint8[N][K][nq]: K >= 1 chains per syndrome that all have that syndrome (not checked: e.g. the lifted chain, final rung
 * states); target int32[N]: the class the correction shall lie in, in the convention of qecmc_eq_class (the column order of counts /
 * distr: argmax of a row).  corrections_out uint8[N][nq]: a chain with the candidates' syndrome in class target -- the lightest
 * candidate already in that class (lowest index on ties; moved 0), else the lightest of all (moved 1) multiplied by the logical
 * operators a host-derived class-move table names (csrc/corrections.hpp), each at position 0 (place == 0) or at the position in
 * [0, L) that gives the lowest error count (place != 0, ties to the lowest position); descend != 0 then runs the greedy descent of
 * qecmc_chains_from_syndromes.  weight_out int32[N]: count_errors of the correction; source_out int32[N]: the candidate it came
 * from; moved_out uint8[N]; status_out uint8[N]: 0 corrected, 1 target outside [0, ncls) -- that chain is all zero, weight -1,
 * source -1, moved 0.  The last four are nullable.
 * Additive: QECMC_ABI_VERSION stays.  A NULL required buffer, K == 0 or a (code, L) the library does not know is refused
 * (QECMC_ERR_INVALID), a (code, L) without a class move -- the toric code at even L, whose parity class does not see a logical
 * line -- with QECMC_ERR_UNSUPPORTED, both before a device is looked for.  N == 0 succeeds.
 * qecmc_corrector: the uploaded mask rows, class-move table and generator table of one (code, L), on the device current when it was
 * created.  The _dev form takes device pointers and a hipStream_t, allocates nothing and does not synchronise (it composes on one
 * stream with qecmc_generate_syndromes_dev, qecmc_chains_from_syndromes_dev and qecmc_pteq_launch_dev); the corrector must outlive
 * the launches enqueued with it. */
int qecmc_corrections(int code, int L, uint64_t N, uint32_t K, const uint8_t *candidates, const int32_t *target, int place,
                      int descend, uint8_t *corrections_out, int32_t *weight_out, int32_t *source_out, uint8_t *moved_out,
                      uint8_t *status_out);
typedef struct qecmc_corrector qecmc_corrector;
int qecmc_corrector_create(int code, int L, qecmc_corrector **out);
int qecmc_corrector_destroy(qecmc_corrector *c);
int qecmc_corrections_dev(qecmc_corrector *c, const void *d_candidates, const void *d_target, uint64_t N, uint32_t K, int place,
                          int descend, void *d_corrections_out, void *d_weight_out /*nullable*/, void *d_source_out /*nullable*/,
                          void *d_moved_out /*nullable*/, void *d_status_out /*nullable*/, void *hip_stream);

/* ---- the exact class law by coset enumeration (no counterpart in the reference: every decoder there estimates this) --------------
 * chains uint8[N][nq]: one chain per syndrome (e.g. the lifted chain).  hist_out uint64[N][ncls][nq+1][nq+1]:
 * hist[s][c][n_xy][n_z] = the number of chains with the syndrome of chain s, in class c (the convention of qecmc_eq_class: the column
 * order of counts / distr), that have n_xy X or Y errors and n_z Z errors -- counted over the elements of the stabilizer group the call
 * covers.  Every weight the library knows is a function of (n_xy, n_z): Z_c = sum hist[s][c] * w(n_xy, n_z) is the EXACT weight of
 * class c, and a whole class sums to 2^rank.  class_out int32[N] (nullable): the class of the input chain.
 * Element e in [0, 2^rank) of the group is the product of the basis generators whose bit is set in e, the basis being the generators
 * greedy GF(2) elimination keeps in table order (csrc/enumerate.hpp); chunk k of width chunk_bits (0: the default, at most 24; a value
 * beyond the rank means the rank) is e in [k << chunk_bits, (k + 1) << chunk_bits).  The call covers chunks
 * [chunk_first, chunk_first + chunk_count), chunk_count == 0 meaning all from chunk_first: histograms over disjoint ranges add up to
 * the whole, one launch covers one chunk of a bounded group of syndromes, and hist_out is overwritten, not added to.
 * qecmc_coset_enumerate_info: the sizes of one (code, L) -- every pointer nullable --, on the host alone.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for: a NULL chains / hist_out, a (code, L) the library does not
 * know (xzzx / rotated at even L among them), chunk_bits outside {0} and [8, 30] or a chunk range past 2^(rank - chunk_bits) with
 * QECMC_ERR_INVALID; more than 32 qubits, a rank above 36 or below 8, a (code, L) without a class move (the toric code at even L) or
 * a histogram beyond the kernel's LDS with QECMC_ERR_UNSUPPORTED -- which leaves toric L = 3, planar L = 3, 4 and xzzx / rotated
 * L = 3, 5.  N == 0 succeeds.  Host pointers only. */
int qecmc_coset_enumerate_info(int code, int L, int32_t *rank, int32_t *ncls, int32_t *nq, int32_t *default_chunk_bits);
int qecmc_coset_enumerate(int code, int L, uint64_t N, const uint8_t *chains, int chunk_bits, uint64_t chunk_first,
                          uint64_t chunk_count, uint64_t *hist_out, int32_t *class_out);

/* ---- the exact class law by a frontier sweep: the same law where 2^rank elements are out of reach -----------------------------------
 * chains uint8[N][nq]: one chain per syndrome.  w[4]: the weight of I, X, Y and Z at one qubit (any positive scale; the library's noise
 * models in ratio form have w[0] = 1), finite and > 0.  z_out double[N][ncls]:
 * z_out[s][c] = the sum over the chains of class c (the convention of qecmc_eq_class) with the syndrome of chain s of prod_q w[Pauli at q]
 * -- the product over the qubits of the code: a cell of the state layout that holds no qubit (the planar code's) does not enter.
 * class_out int32[N] (nullable): the class of the input chain.  The sum is carried out by variable elimination across the lattice
 * (csrc/class_sweep.hpp): (2 G + nq) 2^width operations per class, width the widest frontier of the plan, on a state vector in LDS.
 * qecmc_class_sweep_info: width, ncls, nq and the number of ops of the plan of one (code, L) -- every pointer nullable --, on the host alone.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for: a NULL chains / w / z_out, a weight that is not finite and
 * > 0 or a (code, L) the library does not know with QECMC_ERR_INVALID; a (code, L) without a class move (the toric code at even L) or a
 * plan wider than 13 with QECMC_ERR_UNSUPPORTED -- which leaves toric L = 3, planar L = 3 .. 6 and xzzx / rotated L = 3, 5, 7, 9.
 * N == 0 succeeds.  Host pointers only.  (qecmc_class_sweep_cut below takes the next shapes.)
 * Range: z_out is raw -- what IEEE double arithmetic gives, with no rescaling: about count * f^cost in ratio form, so it may be subnormal
 * (kept, not flushed: the device gives the host twin's bits there too) or 0 at low error rates and large L, and inf under weights above 1.
 * That holds for qecmc_class_sweep_cut, _tiled and the three _site forms below as well.  Whether a row still carries a law is judged where
 * it is normalised (qecmc.exact.law_from_class_weights: refused by name below a row total of 2^-960 and where a weight is not finite). */
int qecmc_class_sweep_info(int code, int L, int32_t *width, int32_t *ncls, int32_t *nq, int32_t *n_ops);
int qecmc_class_sweep(int code, int L, uint64_t N, const uint8_t *chains, const double *w, double *z_out, int32_t *class_out);

/* ---- the frontier sweep past one LDS state vector: cut-set conditioning (csrc/class_sweep_cut.hpp) ------------------------------------
 * The arguments and the result of qecmc_class_sweep, for plans it refuses as too wide.  n_held generators are held out of the elimination:
 * for every assignment h of them the class representative is multiplied by the held generators h names and the rest is swept as before,
 * over a frontier of `width` <= lds_width; z = 2^-(G - rank) * the sum of the 2^n_held partial sweeps, taken in a fixed order.  One (class,
 * syndrome) is 2^n_held workgroups and one workgroup that sums them; a launch covers a bounded group of syndromes, whatever N.
 * lds_width: the widest state vector a workgroup may hold, 2 .. 14 (2^lds_width doubles of LDS; 14 is 128 KiB, one workgroup per CU), or
 * 0 for the default: 13 where nothing is held then, 14 where that holds nothing, else 13.
 * qecmc_class_sweep_cut_info: the frontier of the uncut plan, the cut plan's width, held generators, classes, qubits and ops -- every
 * pointer nullable --, on the host alone.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for: what qecmc_class_sweep refuses with QECMC_ERR_INVALID, and an
 * lds_width outside {0} and [2, 14]; a (code, L) without a class move (the toric code at even L) or a plan that would hold more than 12
 * generators with QECMC_ERR_UNSUPPORTED -- which adds toric L = 5, planar L = 7 and xzzx / rotated L = 11 to qecmc_class_sweep's shapes;
 * toric L >= 7, planar L >= 8 and xzzx / rotated L >= 13 stay refused.  A device that does not grant 128 KiB of LDS to a workgroup
 * answers QECMC_ERR_UNSUPPORTED at width 14.  Where n_held is 0 and width <= 13 the result is qecmc_class_sweep's, bit for bit.
 * N == 0 succeeds.  Host pointers only. */
int qecmc_class_sweep_cut_info(int code, int L, int lds_width, int32_t *full_width, int32_t *width, int32_t *n_held, int32_t *ncls,
                               int32_t *nq, int32_t *n_ops);
int qecmc_class_sweep_cut(int code, int L, uint64_t N, const uint8_t *chains, const double *w, int lds_width, double *z_out,
                          int32_t *class_out);

/* ---- the frontier sweep on a state vector tiled over HBM (csrc/class_sweep_tiled.hpp) -------------------------------------------------
 * The arguments and the result of qecmc_class_sweep_cut, for frontiers no LDS state vector holds.  The state vector of one (syndrome, class,
 * assignment) is 2^width doubles in a device workspace (1 GiB at most, whatever N), width <= hbm_width; the op stream is cut into segments
 * whose INTRO / FORGET slots fit tile_width index bits, and one launch per segment moves every live tile of 2^tile_width doubles through
 * LDS.  Where the frontier is wider than hbm_width, n_held generators are held out by qecmc_class_sweep_cut's rule and summed over in its
 * order.  hbm_width: tile_width .. 24 (128 MiB per state vector), 0 for the default, 24.  tile_width: 4 .. 13, 0 for the default, 11 (the fastest measured).
 * qecmc_class_sweep_tiled_info: the frontier of the plan with nothing held, the plan's width, held generators, classes, qubits, ops and
 * segments -- every pointer nullable --, on the host alone.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for: what qecmc_class_sweep refuses with QECMC_ERR_INVALID, and an
 * hbm_width or tile_width out of range; a (code, L) without a class move (the toric code at even L) or a frontier that 12 held generators
 * do not bring down to hbm_width with QECMC_ERR_UNSUPPORTED, by name with its widths -- which adds planar L = 8 .. 12, xzzx / rotated
 * L = 13 .. 21 and toric L = 7 to qecmc_class_sweep_cut's shapes; toric L >= 9 (37 wide), planar L >= 13 and xzzx / rotated L >= 23 (26
 * wide) stay refused.  The result is the same bits for every tile_width;
 * where nothing is held and width <= 13 it is qecmc_class_sweep's, and where the held generators are qecmc_class_sweep_cut's (hbm_width =
 * its lds_width) it is that one's, bit for bit.  Denormal entries are kept on either side.  N == 0 succeeds.  Host pointers only. */
int qecmc_class_sweep_tiled_info(int code, int L, int hbm_width, int tile_width, int32_t *full_width, int32_t *width, int32_t *n_held,
                                 int32_t *ncls, int32_t *nq, int32_t *n_ops, int32_t *n_segments);
int qecmc_class_sweep_tiled(int code, int L, uint64_t N, const uint8_t *chains, const double *w, int hbm_width, int tile_width,
                            double *z_out, int32_t *class_out);

/* ---- the three sweeps under a weight per (syndrome, qubit): erasures, inhomogeneous noise, soft priors (csrc/class_sweep_site.hpp) ------
 * The arguments and the result of qecmc_class_sweep, qecmc_class_sweep_cut and qecmc_class_sweep_tiled with the four weights w replaced by a
 * table: wq double[wq_rows][nq][4], the weights of I, X, Y and Z at every cell of the state layout (any non-negative scale per qubit; in
 * ratio form w_I = 1).  wq_rows is 1 -- one table for every syndrome -- or N -- row s belongs to syndrome s: a shot's own erased qubits carry
 * (1, 1, 1, 1).  z_out[s][c] = the sum over the chains of class c with the syndrome of chain s of prod_q wq[row(s)][q][Pauli at q].
 * Plans, widths, holds, segments and launch groups are the sibling's -- its _info call reports them, and what it accepts and refuses is what
 * the site entry point accepts and refuses, with the same code and message.  The device holds the weight rows of one launch group at a time.
 * Weights are finite and >= 0: zero is allowed (off an erased set the pure-erasure limit is (1, 0, 0, 0)), the arithmetic stays copies,
 * multiplies and adds of finite non-negative numbers -- which stay finite for weights <= 1; weights above 1 can take z_out to inf.  Only the rows of qubits the plan closes are read: a cell that holds no qubit (the planar
 * code's unused cells) is neither read nor validated.  With constant rows the result is the uniform sibling's, bit for bit.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, with QECMC_ERR_INVALID: everything the sibling refuses so, a
 * NULL wq, a wq_rows that is neither 1 nor N (N > 0), a weight that is negative, NaN or infinite -- by row, qubit and Pauli --, a qubit whose
 * four weights are all zero; with QECMC_ERR_UNSUPPORTED: the sibling's (code, L) and width refusals.  N == 0 succeeds.  Host pointers only. */
int qecmc_class_sweep_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, double *z_out,
                           int32_t *class_out);
int qecmc_class_sweep_cut_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int lds_width,
                               double *z_out, int32_t *class_out);
int qecmc_class_sweep_tiled_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int hbm_width,
                                 int tile_width, double *z_out, int32_t *class_out);

/* ---- the shortest chain of every class and its multiplicity: the sweep in the (min, +, count) semiring (csrc/class_minplus.hpp) --------
 * chains, N, lds_width and class_out as qecmc_class_sweep_cut takes them; the plans are that entry point's, unchanged, and
 * qecmc_class_sweep_cut_info reports them.  cost[4]: the integer cost of I, X, Y and Z at one qubit, 0 .. 255 each; zero is allowed anywhere
 * and so is a non-zero cost of I.  cost_out uint32[N][ncls]: cost_out[s][c] = the least sum over the qubits of cost[Pauli at q] among the
 * chains of class c with the syndrome of chain s -- a cell that holds no qubit (the planar code's) does not enter; count_out uint64[N][ncls]:
 * the number of chains of that class that reach it.  Integer arithmetic throughout: the result is exact and depends on the syndrome alone.
 * A count is kept in 48 bits while the generator table is swept (every chain is met 2^(G - rank) times there: 4 on the torus); one that
 * reaches 2^48 - 1 saturates, stays saturated and is reported as count_out = 0 -- a true count is never 0.
 * At cost = (0, 1, 1, 1) the class of least cost is the minimum-weight decoder of depolarizing noise over Pauli chains (a Y costs 1).
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, the message prefixed "qecmc_class_minplus:": a NULL chains /
 * cost / cost_out / count_out or a cost above 255 with QECMC_ERR_INVALID, and whatever qecmc_class_sweep_cut refuses, with its code -- which
 * leaves toric L = 3, 5, planar L = 3 .. 7 and xzzx / rotated L = 3 .. 11.  A device that does not grant 128 KiB of LDS to a workgroup answers
 * QECMC_ERR_UNSUPPORTED at width 14.  N == 0 succeeds.  Host pointers only. */
int qecmc_class_minplus(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t cost[4], int lds_width, uint32_t *cost_out,
                        uint64_t *count_out, int32_t *class_out);

/* ---- a shortest chain of every class: the (min, +) sweep traced back (csrc/class_minplus_trace.hpp) --------
 * The arguments and shapes of qecmc_class_minplus, and one more output: chain_out uint8[N][ncls][nq], chain_out[s][c] a chain with the
 * syndrome of chain s, in class c, whose cost is cost_out[s][c] -- bytes 0 .. 3 for I, X, Y, Z, the format of the input; a cell no
 * generator touches keeps the byte of the class representative.  cost_out and count_out are qecmc_class_minplus's, exactly; they and
 * class_out may be NULL.  The chain is a function of (plan, input chain, cost) alone.  Where count_out == 1 it is the one shortest chain
 * of the class and depends on the syndrome alone; where several chains tie, the one returned is selected by a fixed rule (of the
 * assignments of the held generators the lowest that reaches the least cost; a generator is applied only where that is strictly
 * cheaper) FROM THE INPUT CHAIN: another chain with the same syndrome may select another of the tied chains.  A saturated count does not
 * touch the chain.  Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, the message prefixed
 * "qecmc_class_minplus_chains:": what qecmc_class_minplus refuses, with its codes (a NULL chains / cost / chain_out here).  N == 0
 * succeeds.  Host pointers only; device 0. */
int qecmc_class_minplus_chains(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t cost[4], int lds_width, uint8_t *chain_out,
                               uint32_t *cost_out, uint64_t *count_out, int32_t *class_out);

/* ---- both under a cost per (syndrome, qubit): erasures, inhomogeneous noise, soft priors on an integer scale (csrc/class_minplus_site.hpp) ----
 * The arguments, shapes, nullability and results of qecmc_class_minplus and qecmc_class_minplus_chains with the four costs replaced by a
 * table: cq uint8[cq_rows][nq][4], the costs of I, X, Y and Z at every cell of the state layout, every byte value a cost.  cq_rows is 1 -- one
 * table for every syndrome -- or N -- row s belongs to syndrome s: a shot's own erased qubits cost (0, 0, 0, 0).  cost_out[s][c] = the least
 * sum over the qubits of cq[row(s)][q][Pauli at q] among the chains of class c with the syndrome of chain s, count_out[s][c] the number of
 * chains that reach it, chain_out[s][c] one of them, selected by qecmc_class_minplus_chains' rule.  With integer log-likelihood costs that is
 * the most likely chain of the class, exactly.  Plans, widths, holds and launch groups are the siblings'; the device holds the cost rows of one
 * launch group at a time.  Only the rows of qubits the plan closes are read: a cell that holds no qubit (the planar code's unused cells) may
 * hold anything.  With constant rows the result is the uniform sibling's, chains included.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, the message prefixed "qecmc_class_minplus_site:" /
 * "qecmc_class_minplus_chains_site:": what the sibling refuses of (code, L, N, lds_width), with its codes; a NULL chains / cq / output the
 * sibling requires and a cq_rows that is neither 1 nor N (N > 0) with QECMC_ERR_INVALID.  N == 0 succeeds.  Host pointers only; device 0. */
int qecmc_class_minplus_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int lds_width,
                             uint32_t *cost_out, uint64_t *count_out, int32_t *class_out);
int qecmc_class_minplus_chains_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int lds_width,
                                    uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out, int32_t *class_out);

/* ---- exact chains of every class: the traced sum-product sweep, forward filtering and backward sampling (csrc/class_sample.hpp) --------
 * chains, N, lds_width and the plans are qecmc_class_sweep_cut's; w[4] / wq, wq_rows are that function's and qecmc_class_sweep_cut_site's, except
 * that the four weights may hold zeros (finite and >= 0, not all zero).  K: samples per syndrome (mode 1) or per (syndrome, class) (mode 0),
 * 1 .. 2^32 - 1.  mode 0, every class: chain_out uint8[N][ncls][K][nq], chain_out[s][c][k] a chain with the syndrome of chain s, in class
 * c, drawn with probability w(chain) / Z_c; class_out is not looked at.  mode 1, posterior: the class is drawn first with probability
 * Z_c / Z -- class_out int32[N][K] -- and chain_out uint8[N][K][nq] is sample (s, class_out[s][k], k) of mode 0.  z_out double[N][ncls] in
 * both modes: qecmc_class_sweep_cut's bits.  Bytes 0 .. 3 are I, X, Y, Z; a cell no generator touches keeps the byte of the class
 * representative.  A sample is a function of (seed, first_syndrome + s, c, k, the plan, chain s, the weights) alone -- not of N, K or the
 * batch around it -- drawn from Philox sub-stream 0x53 (DESIGN.md "RNG addressing"); each branch is taken with its probability up to 2^-53.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, the message prefixed "qecmc_class_sample:" /
 * "qecmc_class_sample_site:": a NULL chains / w / wq / chain_out / z_out (class_out in mode 1), K = 0 or K >= 2^32, first_syndrome + N past
 * 2^32, a mode other than 0 and 1, a weight that is negative or not finite, and whatever qecmc_class_sweep_cut / _cut_site refuses, with its
 * code.  Refused once z is known, with QECMC_ERR_INVALID: in mode 0 a class whose weight is 0, not finite or below 2^-960 (the sweep is not
 * rescaled: below that the record is rounded in the subnormal range and the draws would not follow the law), by row and class; in mode 1 a
 * row whose total is.  A drawn chain has weight > 0 at every range.  N == 0 succeeds.  Host pointers only; device 0. */
int qecmc_class_sample(int code, int L, uint64_t N, const uint8_t *chains, const double w[4], int lds_width, uint64_t K, uint64_t seed,
                       uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out);
int qecmc_class_sample_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int lds_width, uint64_t K,
                            uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out);

/* ---- exact per-qubit marginals of every class: forward filtering and a backward sum on the cut-set sweep (csrc/class_marginal.hpp) --------
 * chains, N, lds_width and the plans are qecmc_class_sweep_cut's; w[4] / wq, wq_rows are qecmc_class_sample's / _sample_site's: finite and >= 0,
 * zeros allowed, not all zero.  weights_out double[N][ncls][nq][4]: weights_out[s][c][q][P] is the sum of w(chain) over the chains of class c
 * with the syndrome of chain s that carry Pauli P (I, X, Y, Z) at cell q, so weights_out / z_out is P(q carries P | syndrome, class) and the
 * four sum to z_out[s][c] up to rounding.  A cell no generator touches gets z_out[s][c] at the byte of the class representative and 0
 * elsewhere.  z_out double[N][ncls]: qecmc_class_sweep_cut's bits.  class_out int32[N] (nullable): the class of every input chain.  Every
 * number is a sum of products of non-negative doubles in an order that is a function of the plan alone (THE RULE of class_marginal.hpp): no
 * subtraction, no division; a weight of 0 gives exact zeros.  The device holds the forward records of 512 MiB of jobs at a time, whatever N.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, the message prefixed "qecmc_class_marginals:" /
 * "qecmc_class_marginals_site:": a NULL chains / w / wq / weights_out / z_out, N past 32 bits, a weight that is negative or not finite, four
 * zero weights, and whatever qecmc_class_sweep_cut / _cut_site refuses, with its code.  N == 0 succeeds.  Host pointers only; device 0. */
int qecmc_class_marginals(int code, int L, uint64_t N, const uint8_t *chains, const double w[4], int lds_width, double *weights_out,
                          double *z_out, int32_t *class_out);
int qecmc_class_marginals_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int lds_width,
                               double *weights_out, double *z_out, int32_t *class_out);

/* ---- the (min, +, count) sweep on the state vector tiled over HBM: xzzx / rotated L = 13 .. 21, planar L = 8 .. 12, toric L = 7
 * (csrc/class_minplus_tiled.hpp) ----
 * The arguments and results of qecmc_class_minplus and qecmc_class_minplus_site -- cost_out uint32[N][ncls], count_out uint64[N][ncls] (0 where
 * saturated), class_out int32[N] (nullable) -- on the plans of qecmc_class_sweep_tiled: hbm_width and tile_width are that function's, and
 * qecmc_class_sweep_tiled_info gives the plan's facts.  The result does not depend on tile_width, and where the holds are the cut plan's
 * (hbm_width = its lds_width) it is qecmc_class_minplus's.  qecmc_class_minplus_tiled_chains (below) traces a chain back.
 * The 16 bits of an entry's cost do not cover 255 per qubit at these shapes, so the cost range is checked per call: n_qubits * max(cost) < 2^16,
 * and for a table the sum over the plan's qubits of a row's largest cost at the qubit < 2^16 in every row (QECMC_ERR_UNSUPPORTED, the row named).
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, the message prefixed "qecmc_class_minplus_tiled:" /
 * "qecmc_class_minplus_tiled_site:": a NULL chains / cost / cq / cost_out / count_out, N beyond 32 bits, a cost above 255, a cq_rows that is
 * neither 1 nor N (N > 0) with QECMC_ERR_INVALID; what qecmc_class_sweep_tiled refuses of (code, L, hbm_width, tile_width), with its codes; the
 * cost range.  N == 0 succeeds.  Host pointers only; device 0. */
int qecmc_class_minplus_tiled(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t cost[4], int hbm_width, int tile_width,
                              uint32_t *cost_out, uint64_t *count_out, int32_t *class_out);
int qecmc_class_minplus_tiled_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int hbm_width,
                                   int tile_width, uint32_t *cost_out, uint64_t *count_out, int32_t *class_out);

/* ---- a shortest chain of every class on the tiled route: the tiled (min, +) sweep traced back (csrc/class_minplus_tiled_trace.hpp) ----
 * qecmc_class_minplus_chains and qecmc_class_minplus_chains_site on the plans of qecmc_class_minplus_tiled: chain_out uint8[N][ncls][nq] --
 * chain_out[s][c] has the syndrome of chain s, lies in class c and costs cost_out[s][c] --; cost_out, count_out and class_out are nullable and exactly
 * those of qecmc_class_minplus_tiled / _site.  The chain is a pure function of (plan's stream and holds, representative, costs) under the tie rule
 * of qecmc_class_minplus_chains: it does not depend on tile_width, and where the tiled plan's stream and holds are the cut plan's it is that
 * function's chain byte for byte.  One more tiled pass per (syndrome, class) pair records one decision bit per FORGET and live state in a device
 * block of its own, 2 GiB at most, kept per device; a plan whose single pair takes more is refused by name with its bytes.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, the message prefixed "qecmc_class_minplus_tiled_chains:" /
 * "qecmc_class_minplus_tiled_chains_site:": a NULL chains / cost / cq / chain_out, N beyond 32 bits, and whatever qecmc_class_minplus_tiled / _site
 * refuses, with its code -- the cost range included.  N == 0 succeeds.  Host pointers only; device 0. */
int qecmc_class_minplus_tiled_chains(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t cost[4], int hbm_width, int tile_width,
                                     uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out, int32_t *class_out);
int qecmc_class_minplus_tiled_chains_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int hbm_width,
                                          int tile_width, uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out, int32_t *class_out);

/* ---- exact chains of every class on the tiled route: forward filtering and backward sampling on the state vector tiled over HBM
 * (csrc/class_sample_tiled.hpp) ----
 * qecmc_class_sample and qecmc_class_sample_site on the plans of qecmc_class_sweep_tiled: K, seed, first_syndrome, mode, chain_out, class_out
 * (not looked at in mode 0; required in mode 1) and z_out are those functions', hbm_width and tile_width are qecmc_class_sweep_tiled's, and
 * z_out is qecmc_class_sweep_tiled's bits.  A sample is a function of (seed, first_syndrome + s, c, k, the plan's stream and holds, chain s,
 * the weights) alone: it does not depend on tile_width, N, K or record_bytes, and where the tiled plan's stream and holds are the cut plan's
 * (hbm_width = its lds_width) it is qecmc_class_sample's chain byte for byte.  One more tiled pass per job -- a (syndrome, class) pair, or with
 * held generators a (syndrome, class, sample) triple -- records 16 bytes per FORGET and live state in a device block of its own, kept per
 * device.  record_bytes caps the block of one call: 0 is the default of 4 GiB (xzzx / rotated up to L = 17), other values are taken up to
 * 64 GiB; a block grown past the default is freed before the call returns.  A plan whose single job takes more than the cap is refused by
 * name with the bytes it needs (rotated L = 21: about 39 GB).
 * qecmc_class_sample_tiled_info: n_forget, bytes_per_job and jobs_per_pass (all three (nullable)) of the plan under that cap -- the FORGETs of
 * the stream, the record of one job, and the jobs one record pass carries when many are left; a plan refused for the cap alone still reports
 * the first two before it returns the refusal.
 * Additive: QECMC_ABI_VERSION stays.  Refused before a device is looked for, the message prefixed "qecmc_class_sample_tiled:" /
 * "qecmc_class_sample_tiled_site:": a NULL chains / w / wq / chain_out / z_out (class_out in mode 1); what qecmc_class_sample refuses of
 * (N, K, first_syndrome, mode, weights); a record_bytes above 64 GiB; what qecmc_class_sweep_tiled / _tiled_site refuses of (code, L,
 * hbm_width, tile_width, wq, wq_rows), with its codes; the record cap (QECMC_ERR_UNSUPPORTED).  Refused once z is known, as
 * qecmc_class_sample: a class weight (mode 0) or a row total (mode 1) that is 0, not finite or below 2^-960.  N == 0 succeeds.  Host
 * pointers only; device 0. */
int qecmc_class_sample_tiled(int code, int L, uint64_t N, const uint8_t *chains, const double w[4], int hbm_width, int tile_width,
                             uint64_t record_bytes, uint64_t K, uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out,
                             int32_t *class_out, double *z_out);
int qecmc_class_sample_tiled_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int hbm_width,
                                  int tile_width, uint64_t record_bytes, uint64_t K, uint64_t seed, uint32_t first_syndrome, int mode,
                                  uint8_t *chain_out, int32_t *class_out, double *z_out);
int qecmc_class_sample_tiled_info(int code, int L, int hbm_width, int tile_width, uint64_t record_bytes, int32_t *n_forget,
                                  uint64_t *bytes_per_job, uint32_t *jobs_per_pass);

/* ---- chain / ladder on caller-owned state (host pointers) ----------------- */

/* The supported range of a start index.  A Philox counter holds a proposal index (the swap stream: a ladder-step index) in 48 bits,
 * so the entry points that take one -- k0 of qecmc_chain_update*, step0 / prop0 of qecmc_ladder_step*, step0 of qecmc_pteq_resume_dev
 * and qecmc_pteq_resume_conv_dev (whose first proposal is step0 * iters) -- return QECMC_ERR_INVALID, before anything is enqueued, when
 * the index of the call's last proposal (or ladder step) plus 64 is not below 2^48, or when step0 * iters or
 * prop0 + nsteps * iters overflows 64 bits: indices there would draw the blocks of index - 2^48 again (DESIGN.md "RNG addressing"). */

/* Chain.update_chain(iters), src/mcmc.py:19-43, on N independent chains.
 * Chain i draws from Philox stream (syndrome = first_syndrome+i, slot, proposals
 * k0 .. k0+iters-1).  p_logical != 0 selects the top-chain branch (mcmc.py:20). */
int qecmc_chain_update(int code, int L, uint64_t N, uint8_t *states_inout, double p, double p_logical,
                       uint64_t iters, uint64_t seed, uint32_t first_syndrome, uint32_t slot, uint64_t k0);

/* Chain_biased.update_chain(iters), src/mcmc_biased.py:20-59 (acceptance pn/pb from the full
 * (nx,ny,nz) counts, pb frozen at loop entry as in the reference, quirk Q3). */
int qecmc_chain_update_biased(int code, int L, uint64_t N, uint8_t *states_inout, double p, double eta,
                              double p_logical, uint64_t iters, uint64_t seed, uint32_t first_syndrome,
                              uint32_t slot, uint64_t k0);

/* Chain_alpha.update_chain(iters), src/mcmc_alpha.py:27-70: the biased rule with (p_x, p_y, p_z) derived from
 * (pz_tilde, alpha).  accepted_out uint8[N] (nullable) = 1 iff chain i accepted at least one proposal -- the
 * reference refreshes the chain's n_eff attribute on accepted moves only (:58,:70). */
int qecmc_chain_update_alpha(int code, int L, uint64_t N, uint8_t *states_inout, double pz_tilde, double alpha,
                             double p_logical, uint64_t iters, uint64_t seed, uint32_t first_syndrome,
                             uint32_t slot, uint64_t k0, uint8_t *accepted_out);

/* Chain_xyz.update_chain_fast(iters), src/mcmc.py:106-114,162-173 (what decoders.py:352,442 sample STDC_general_noise with): a
 * generator proposal accepted with probability prod_i (p_i / (1 - p_x - p_y - p_z))^(change of n_i), i = x, y, z; p_xyz double[3]. */
int qecmc_chain_update_xyz(int code, int L, uint64_t N, uint8_t *states_inout, const double *p_xyz, uint64_t iters,
                           uint64_t seed, uint32_t first_syndrome, uint32_t slot, uint64_t k0);

/* Ladder.step(iters) x nsteps, src/mcmc.py:94-103, on N ladders in slot order.
 * states uint8[N][Nc][nq], flags uint8[N][Nc], tops0 uint32[N]; step0 / prop0 =
 * ladder steps / proposals per slot already done (Philox addressing: at ladder step T the top chain draws from
 * stream Nc-1, the chain on a lower slot c from the "diagonal" stream 0x400 + (c + T) mod Nc).  Uses
 * params->{code,L,Nc,p,p_logical,seed,first_syndrome,device}. */
int qecmc_ladder_step(const qecmc_params *params, uint64_t N, uint8_t *states_inout, uint8_t *flags_inout,
                      uint32_t *tops0_inout, uint64_t iters, uint64_t nsteps, uint64_t step0, uint64_t prop0);

/* Ladder_alpha.step(iters) x nsteps, src/mcmc_alpha.py:127-137 (params->noise = QECMC_NOISE_ALPHA, params->p =
 * pz_tilde_bottom, params->alpha).  neff_counts_inout uint16[N][Nc][2] carries each SLOT's n_eff attribute as the
 * pair (n_z, n_x + n_y) it was last computed from (n_eff = n_z + alpha (n_x + n_y), :58): the reference swaps codes
 * and flags but not n_eff, so the attribute can lag the slot's configuration and is state the
 * caller must carry between calls. */
int qecmc_ladder_step_alpha(const qecmc_params *params, uint64_t N, uint8_t *states_inout, uint8_t *flags_inout,
                            uint32_t *tops0_inout, uint16_t *neff_counts_inout, uint64_t iters, uint64_t nsteps,
                            uint64_t step0, uint64_t prop0);

/* ---- the batched hot path: decoders.PTEQ (decoders.py:25-89) on N syndromes */

/* Host-pointer form.  init uint8[N][nq] (one seed configuration per syndrome,
 * generate_data.py:131-138); counts_out uint32[N][ncls] = eq[since_burn]
 * (decoders.py:66-67); samples_out uint32[N] = since_burn+1 or 0 when the burn-in
 * never ended (A10 "burn-in trap"); tops0_out uint32[N] (nullable);
 * steps_done_out uint32[N] (nullable) = ladder steps run until the convergence
 * criterion fired (decoders.py:74-82), or params->steps; converged_out uint8[N]
 * (nullable); final_states_out uint8[N][Nc][nq] in slot order (nullable; only
 * meaningful with conv_mode NONE); stats nullable.
 * conv_mode ERROR_BASED needs device workspace for the per-step bottom-chain error counts the criterion averages
 * (decoders.py:68,93-105): 2*N*steps bytes (alpha noise: 4, the two counts behind n_eff), or -- for the ladders that run on a
 * persistent grid with a work queue (a lane whose ladder has stopped takes the next one of the batch in place: the depolarizing
 * random-scan ladders of every code with a top rung at p = 0.75, toric L <= 16 and the others L <= 32, and the biased / alpha rules
 * on the xzzx / rotated codes) -- the same per min(N, grid*64) columns.  A plan's queue counter is its own: one launch of a
 * conv_mode plan at a time. */
int qecmc_pteq_batch(const qecmc_params *params, const uint8_t *init, uint64_t N, uint32_t *counts_out,
                     uint32_t *samples_out, uint32_t *tops0_out, uint32_t *steps_done_out,
                     uint8_t *converged_out, uint8_t *final_states_out, qecmc_stats *stats_out);

/* PTDC (decoders.py:168-233, conv_mult = 0) on N syndromes: the direct-counting estimator.  For every syndrome and
 * class, `droplets` independent ladders WITHOUT logical moves (decoders.py:182,196) run params->steps ladder steps of
 * params->iters proposals at p = params->p (p_sampling); after every step every rung's configuration goes into the
 * (syndrome, class) set of chains seen so far (PTDC_droplet, decoders.py:146-152; the droplets' sets are merged,
 * :220-226).  init uint8[N][ncls][nq] = one representative per class (what the reference's list form of init_code /
 * to_class provides); hist_out uint32[N][ncls][nq+1] = N(n), the number of distinct chains of each length found.
 * The caller forms Z_E = sum_n N(n) exp(-beta n) with beta from p_error (:208,229-233).  PTDC itself passes
 * steps // Nc (:201).  Ladder l = (s * ncls + c) * droplets + d draws from Philox syndrome first_syndrome + l.
 * Uses params->{code,L,Nc,p,iters,steps,seed,first_syndrome,device}; p_logical is ignored (0).
 * STDC / STDC_droplet (decoders.py:236-322) is the same computation on 1-chain ladders: Nc = 1, iters = 5
 * (`chain.update_chain_fast(5)`, :250).
 * flags: QECMC_PTDC_INIT_PER_DROPLET -- init is uint8[N][ncls][droplets][nq], a start of its own for every droplet
 *        (STDC's "rain", `apply_stabilizers_uniform` per droplet, :246-247);
 *        QECMC_PTDC_SET_PER_RUNG -- one set per (ladder, rung) instead of per (syndrome, class): PTRC_droplet's
 *        per-rung dictionaries (decoders.py:584-631); the outputs are then uint32[N][ncls][droplets][Nc][nq+1].
 * m_out (nullable, shaped like hist_out): m(n), the number of OBSERVATIONS of chains of length n (the len_counts of
 * PTRC_droplet :606-618 and STRC_droplet :768-776), from which the host forms the STRC / PTRC estimates. */
enum { QECMC_PTDC_INIT_PER_DROPLET = 1, QECMC_PTDC_SET_PER_RUNG = 2 };
int qecmc_ptdc_batch(const qecmc_params *params, const uint8_t *init, uint64_t N, int32_t droplets,
                     uint32_t flags, uint32_t *hist_out, uint32_t *m_out, qecmc_stats *stats_out);

/* The same with the `conv_mult` early stop of PTDC_droplet (decoders.py:153-162), STDC_droplet (:256-262) and STRC_droplet
 * (:783-826): whenever a ladder step finds a chain that is new to the DROPLET's own dictionary and no longer than the
 * shortest it has seen (initially 2 L^2, :140), stop = step * conv_mult; the droplet records nothing after the first step
 * with step >= stop and step * 100 >= params->steps.  conv_mult = 0 is qecmc_ptdc_batch.  With QECMC_PTDC_SET_PER_RUNG
 * conv_mult is ignored, as PTRC_droplet's stop is commented out in the reference (:627-630).
 * steps_done_out (nullable) uint32[N][ncls][droplets]: ladder steps each droplet recorded.  A workgroup of 64 droplets
 * leaves the step loop once all of them have stopped. */
int qecmc_ptdc_batch_conv(const qecmc_params *params, const uint8_t *init, uint64_t N, int32_t droplets,
                          uint32_t flags, double conv_mult, uint32_t *hist_out, uint32_t *m_out,
                          uint32_t *steps_done_out, qecmc_stats *stats_out);

/* The same sampling for the general-noise estimators STDC_general_noise / STDC_general_noise_shortest (decoders.py:345-507)
 * and STDC_Nall_n_alpha's weighting (:537-581): xyz_out (nullable) uint32[N][ncls][params->steps * Nc * droplets] receives,
 * for every (syndrome, class) set, n_x | n_y << 10 | n_z << 20 of each DISTINCT chain (count_errors_xyz,
 * planar_model.py:225-229 -- the values of STDC_droplet_general_noise's dict, decoders.py:339-340), in no particular
 * order, the unused tail 0xFFFFFFFF; xyz_count_out (nullable) uint32[N][ncls] their number.  Not with
 * QECMC_PTDC_SET_PER_RUNG.
 * p_xyz_sampling (nullable) double[3]: sample with Chain_xyz (src/mcmc.py:106-114,162-173) instead of Chain -- a single
 * chain (params->Nc must be 1; params->p is ignored) whose proposals are accepted with probability
 * prod_i (p_i / (1 - sum p))^(change of n_i); planar, xzzx and rotated codes (the reference's runs the planar stencil).
 * params->noise = QECMC_NOISE_ALPHA (with params->alpha, params->p = pz_tilde_sampling, Nc = 1, iters = 5) samples with
 * Chain_alpha instead: STDC_droplet_alpha / STDC_Nall_n_alpha (decoders.py:510-581), whose weights
 * n_z + alpha (n_x + n_y) the caller forms from xyz_out. */
int qecmc_ptdc_batch_xyz(const qecmc_params *params, const uint8_t *init, uint64_t N, int32_t droplets,
                         uint32_t flags, double conv_mult, const double *p_xyz_sampling, uint32_t *hist_out,
                         uint32_t *m_out, uint32_t *steps_done_out, uint32_t *xyz_out, uint32_t *xyz_count_out,
                         qecmc_stats *stats_out);

/* Plan + device-pointer form: build once (validates, uploads threshold tables),
 * then launch asynchronously on a caller stream with buffers already in HBM.
 * d_workspace / workspace_bytes: the criterion runs' log (decoders.py:68: nbr_errors_bottom_chain), qecmc_plan_workspace_bytes() bytes
 * -- 0 for conv_mode NONE, then NULL / 0 is fine.  ABI 4: the size travels with the pointer and a buffer smaller than the launch
 * needs is refused (QECMC_ERR_INVALID) before anything is enqueued; the library has ONE formula for it (capi.hip workspace_need). */
typedef struct qecmc_plan qecmc_plan;
int qecmc_plan_create(const qecmc_params *params, qecmc_plan **plan_out);
int qecmc_plan_destroy(qecmc_plan *plan);
/* the workspace a launch of N syndromes needs: with_final_states != 0 for a launch that passes d_final_states (one log column per ladder:
 * 2 N steps bytes, 4 for alpha noise); 0 for one that does not -- the plans with a work queue then log one column per lane of their
 * persistent grid, however large the batch */
int qecmc_plan_workspace_bytes(const qecmc_plan *plan, uint64_t N, int with_final_states, uint64_t *bytes_out);
int qecmc_pteq_launch_dev(qecmc_plan *plan, const void *d_init, uint64_t N, uint32_t first_syndrome,
                          void *d_counts, void *d_samples, void *d_tops0 /*nullable*/,
                          void *d_steps_done /*nullable*/, void *d_converged /*nullable*/,
                          void *d_final_states /*nullable*/, void *d_workspace /*nullable*/, uint64_t workspace_bytes,
                          void *hip_stream);
/* Optional per-syndrome equilibrium observables of the following launches of `plan` (device pointers, either nullable;
 * NULL, NULL switches them off again):
 *   d_swap_accepts uint32[N][Nc-1]: accepted swap tests of rung pair (i, i+1) (Ladder.step's r_flip, src/mcmc.py:96-99);
 *   d_nerr_sums    uint32[N][Nc]:   sum over the ladder steps of count_errors() of the chain in rung c after the step's
 *                                   swaps (what mcmc.py:88-89 reads) -- divide by steps for the time average.
 * Both count every ladder step of the launch (no burn-in) and need nq * steps < 2^32.  Not with replicas > 1.
 * Every scan collects them.  scan = WAVE and scan = COLOUR count in diagnostic kernels of their own (the same chain bit for
 * bit, slower than the fast kernels, which are untouched: DESIGN.md 4.1g): fixed-length runs only, scan = WAVE up to 16 packed
 * state words per rung -- QECMC_ERR_UNSUPPORTED, naming the case, with conv_mode ERROR_BASED or beyond that width. */
int qecmc_plan_set_stats(qecmc_plan *plan, void *d_swap_accepts, void *d_nerr_sums);
/* Continue N ladders for params->steps more ladder steps from caller-held device state (exact continuation: Philox is
 * addressed by step0 = ladder steps already done): d_states uint8[N][Nc][nq] slot order in/out, d_flags uint8[N][Nc] in/out,
 * d_tops0 uint32[N] in/out; d_counts uint32[N][ncls] and d_samples uint32[N] are ADDED to (decoders.py:60-67 bookkeeping
 * continues).  A fresh ladder is d_states[s][c] = init[s] for every rung c, d_flags[s][c] = (c == Nc-1), d_tops0[s] = 0,
 * step0 = 0 (Ladder.__init__, mcmc.py:72-77); chunked runs then reproduce one long run bit for bit.  conv_mode must be NONE. */
int qecmc_pteq_resume_dev(qecmc_plan *plan, void *d_states, void *d_flags, void *d_tops0, uint64_t N,
                          uint32_t first_syndrome, uint64_t step0, void *d_counts, void *d_samples, void *hip_stream);
/* The same for a plan with conv_mode error_based: params->steps more ladder steps of a run that stops each ladder by the
 * criterion (decoders.py:74-105), cut anywhere -- every stop decision and the step it is taken at are those of the one long run.
 * Beside the state of qecmc_pteq_resume_dev the caller holds
 *   d_record     the criterion's per-ladder record (window sums, streak, burn-in, sample count, done flag), record_bytes of
 *                qecmc_plan_resume_conv_bytes(); all zero together with step0 = 0 is a fresh run.  Opaque otherwise: its words are
 *                the kernels' own (some are unused by some kernels); read the run's state from the five outputs below;
 *   d_workspace  the log, log_rows rows of [ceil64(N)] uint16 (alpha noise: uint32), row = the ladder's absolute step, so a longer
 *                run appends rows: log_bytes of qecmc_plan_resume_conv_bytes(); step0 + steps <= log_rows;
 *   d_neff       uint32[N][Nc], the slots' n_eff attributes as n_z | (n_x + n_y) << 16 (alpha noise; NULL otherwise); a fresh ladder: the
 *                counts of init in every rung.
 * d_counts is ADDED to; d_samples, d_tops0, d_steps_done (absolute) and d_converged are the run's totals so far.  A ladder that has
 * stopped keeps its rows of all five; its d_states / d_flags rows are unspecified from then on.
 * scan = random (every rule) and scan = sweep; replicas <= 1; never on the work queue.  Where a fresh launch of the plan runs a kernel that
 * draws the top chain's Philox blocks ahead (3 .. 8 rungs with more than a third of a CU's LDS per workgroup, e.g. toric L >= 12 at Nc = 8,
 * rotated L = 21), the continued launch runs the same kernel without them (as under QECMC_FLAG_NO_PRE): the same results, 20 % more
 * kernel time at toric L = 15, Nc = 8 (profiles/r06_conv_resume_ab.json).
 * Refused before any launch:
 * conv_mode NONE, replicas > 1, a NULL or undersized buffer, step0 + steps > log_rows (QECMC_ERR_INVALID); scan = wave / colour
 * (QECMC_ERR_UNSUPPORTED); no HIP device (QECMC_ERR_NO_DEVICE). */
int qecmc_plan_resume_conv_bytes(const qecmc_plan *plan, uint64_t N, uint64_t log_rows, uint64_t *record_bytes_out,
                                 uint64_t *log_bytes_out);
int qecmc_pteq_resume_conv_dev(qecmc_plan *plan, void *d_states, void *d_flags, void *d_tops0, uint64_t N,
                               uint32_t first_syndrome, uint64_t step0, void *d_counts, void *d_samples,
                               void *d_steps_done, void *d_converged, void *d_record, uint64_t record_bytes,
                               void *d_neff /*alpha noise only*/, void *d_workspace, uint64_t workspace_bytes,
                               uint64_t log_rows, void *hip_stream);
/* Host-pointer qecmc_pteq_batch with the observables of qecmc_plan_set_stats (swap_accepts_out uint32[N][Nc-1],
 * nerr_sums_out uint32[N][Nc]; either nullable). */
int qecmc_pteq_batch_stats(const qecmc_params *params, const uint8_t *init, uint64_t N, uint32_t *counts_out,
                           uint32_t *samples_out, uint32_t *tops0_out, uint32_t *steps_done_out,
                           uint8_t *converged_out, uint8_t *final_states_out, uint32_t *swap_accepts_out,
                           uint32_t *nerr_sums_out, qecmc_stats *stats_out);
/* The shortest-chain statistics of PTEQ_alpha_with_shortest (decoders_biasednoise.py:93-172) for the following launches of
 * `plan`, kept in the kernels (device pointers; all NULL switches them off again).  After every ladder step past burn-in the
 * bottom slot is looked at: c = the class of its configuration, v = its n_eff attribute (the slot's own, as the reference
 * reads it).  Per ladder and class:
 *   d_short_neff double[N][4]: the smallest v seen (100000.0, the reference's sentinel: the class was never seen);
 *   d_short_n    uint32[N][4]: the samples with that v;
 *   d_unique_n   uint32[N][4]: the distinct configurations among them (the size of the reference's `unique` dict);
 *   d_overflow   uint8[N]:     1 if the ladder offered more than set_capacity distinct (configuration, v) pairs to its set --
 *                              its d_unique_n row is then unspecified; other ladders are unaffected.
 * d_set is the ladders' sets, set_bytes >= qecmc_plan_shortest_set_bytes(plan, N, set_capacity) bytes for launches of N
 * syndromes (the launch zeroes it).  Alpha noise with scan = WAVE or scan = COLOUR only, single fresh ladders: any other rule or
 * scan, replicas > 1, or a plan with qecmc_plan_set_stats is refused with QECMC_ERR_UNSUPPORTED, naming the case; a NULL or
 * undersized buffer with QECMC_ERR_INVALID, before anything is enqueued.  Launches run a kernel of their own with one lane (scan
 * = COLOUR: one workgroup) per ladder for the whole run and log one column per ladder (the workspace formula of
 * qecmc_plan_workspace_bytes with final states); conv_mode NONE runs `steps` steps (steps_done = steps, converged = 0);
 * d_tops0, d_steps_done and d_converged are needed, scan = WAVE writes no final states. */
int qecmc_plan_shortest_set_bytes(const qecmc_plan *plan, uint64_t N, uint64_t set_capacity, uint64_t *bytes_out);
int qecmc_plan_set_shortest(qecmc_plan *plan, void *d_short_neff, void *d_short_n, void *d_unique_n, void *d_overflow,
                            void *d_set, uint64_t set_bytes, uint64_t set_capacity);
/* Host-pointer form: qecmc_pteq_batch with the outputs above (none nullable). */
int qecmc_pteq_batch_shortest(const qecmc_params *params, const uint8_t *init, uint64_t N, uint64_t set_capacity,
                              uint32_t *counts_out, uint32_t *samples_out, uint32_t *tops0_out, uint32_t *steps_done_out,
                              uint8_t *converged_out, double *short_neff_out, uint32_t *short_n_out,
                              uint32_t *unique_n_out, uint8_t *overflow_out, qecmc_stats *stats_out);
/* Bytes of dynamic LDS and threads per workgroup the plan's kernel uses (for reports). */
int qecmc_plan_info(const qecmc_plan *plan, uint32_t *lds_bytes, uint32_t *block_threads,
                    uint32_t *syndromes_per_block);

#ifdef __cplusplus
}
#endif
#endif
