// C test API over the host-side table builders (tables.hpp), compiled ALONE by g++ -- no HIP runtime, no device -- with
// -fsanitize=address,undefined (make tables_asan) or plainly (make tables): tests/test_host_tables.py checks every table the
// plan precomputes for the kernels against values the CPU oracle computes; tests/test_kernel_choice.py asks choose_kernel()
// (kernel_choice.hpp) which kernel every shape runs, and plan_host() (plan_host.hpp) which plan -- or which refusal -- a parameter block gets.
// Not part of libqecmc.so.
#include "class_sweep.hpp"
#include "class_sweep_cut.hpp"
#include "class_sweep_tiled.hpp"
#include "class_sweep_site.hpp"
#include "class_minplus.hpp"
#include "class_minplus_trace.hpp"
#include "class_minplus_site.hpp"
#include "class_minplus_tiled.hpp"
#include "class_minplus_tiled_trace.hpp"
#include "class_sample.hpp"
#include "class_marginal.hpp"
#include "class_sample_tiled.hpp"
#include "corrections.hpp"
#include "enumerate.hpp"
#include "kernel_choice.hpp"
#include "plan_host.hpp"
#include "syndrome_lift.hpp"
#include "tables.hpp"
#include "wu_bounds.hpp"
#include "wu_frames.hpp"

#include <cstdio>
#include <cstring>

using namespace qecmc;
using namespace qecmc::tables;

namespace {
template <class T> int put(const std::vector<T> &v, T *out, int cap)
{
    if ((int)v.size() > cap) return -(int)v.size();
    std::memcpy(out, v.data(), v.size() * sizeof(T));
    return (int)v.size();
}
int answer(const Refusal &r, const KernelShape &s, int32_t *shape_ints, char *msg, int msg_cap)
{
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", r.msg.c_str());
    if (!r.code && shape_ints) std::memcpy(shape_ints, &s, sizeof s);
    return r.code;
}
std::vector<uint32_t> gen_table(int code, int L) { return code == QECMC_TORIC ? toric_generator_table(L) : surf_generator_table(code, L); }
}  // namespace

extern "C" {
int qt_generator_table(int code, int L, uint32_t *out, int cap) { return put(gen_table(code, L), out, cap); }
int qt_logical_masks(int code, int L, int W, uint32_t *out, int cap)
{
    return put(code == QECMC_TORIC ? toric_logical_masks(L, W) : surf_logical_masks(code, L, W), out, cap);
}
int qt_wave_descriptors(int code, int L, uint32_t *out, int cap) { return put(wave_descriptors(gen_table(code, L)), out, cap); }
// the wave layout (scan = wave): a qubit's position, the toric descriptors, the logical masks moved to it; qt_plan_wave_tables: wu_desc and lmask
// as plan_host() builds them for an accepted block (the sizes through n_desc / n_lmask; -1: refused or too small a buffer)
uint32_t qt_wave_position(int code, int L, uint32_t q) { return wave_position(code, L, q); }
int qt_toric_wave_descriptors(int L, uint32_t *out, int cap) { return put(toric_wave_descriptors(toric_generator_table(L)), out, cap); }
int qt_wave_logical_masks(int code, int L, int W, uint32_t *out, int cap)
{
    const std::vector<uint32_t> flat = code == QECMC_TORIC ? toric_logical_masks(L, W) : surf_logical_masks(code, L, W);
    return put(wave_layout_rows(code, L, (int)code_nq(code, L), W, flat), out, cap);
}
int qt_plan_wave_tables(const qecmc_params *p, uint32_t *desc, int desc_cap, int *n_desc, uint32_t *lmask, int lmask_cap, int *n_lmask)
{
    HostPlan hp;
    if (validate_params(p).code || plan_host(*p, hp).code) return -1;
    *n_desc = put(hp.wu_desc, desc, desc_cap);
    *n_lmask = put(hp.lmask, lmask, lmask_cap);
    return *n_desc < 0 || *n_lmask < 0 ? -1 : 0;
}
uint64_t qt_thr64(double v) { return thr64(v); }
uint64_t qt_thr44(double v) { return thr44(v); }
uint32_t qt_thr32(double v) { return thr32(v); }
double qt_chain_factor(double p) { return chain_factor(p); }
int qt_ladder(double p_bottom, double p_top, int Nc, double *pl, double *pd)
{
    std::vector<double> a, b;
    ladder_probabilities(p_bottom, p_top, Nc, a, b);
    std::memcpy(pl, a.data(), a.size() * sizeof(double));
    if (!b.empty()) std::memcpy(pd, b.data(), b.size() * sizeof(double));
    return (int)b.size();
}
int qt_bias_tables(int alpha_model, double p, double eta_or_alpha, int nq, double *out, int cap)
{
    return put(alpha_model ? alpha_tables(p, eta_or_alpha, (size_t)nq) : bias_tables(p, eta_or_alpha, (size_t)nq), out, cap);
}
int qt_patterns(int code, int L, uint8_t *gen_type, int cap_types, uint32_t *patterns, int cap_patterns)
{
    std::vector<uint8_t> gt;
    std::vector<uint32_t> pat;
    generator_patterns(gen_table(code, L), gt, pat);
    if (put(gt, gen_type, cap_types) < 0) return -1;
    return put(pat, patterns, cap_patterns);
}
int qt_count_change(const uint32_t *patterns, int n, uint32_t *out, int cap)
{
    return put(count_change_table(std::vector<uint32_t>(patterns, patterns + n)), out, cap);
}
int qt_swap_thresholds(const double *pdiff, int n, int nq, uint64_t *out, int cap)
{
    return put(swap_thresholds(std::vector<double>(pdiff, pdiff + n), nq), out, cap);
}
int qt_colour_phases(int code, int L, uint16_t *out, int cap)
{
    int n_phases = 0;
    const std::vector<uint16_t> ph = colour_phases(gen_table(code, L), n_phases);
    return put(ph, out, cap) < 0 ? -1 : n_phases;
}
// choose_kernel() of n shapes: 11 numbers per shape -- family, maxt, minw, code, flags, wv, conv, it, alpha, rule, why (a const char *)
void qt_choose_kernels(const KernelShape *shapes, int n, int64_t *keys)
{
    for (int i = 0; i < n; ++i) {
        const KernelKey k = choose_kernel(shapes[i]);
        const int64_t v[11] = {k.family, k.maxt, k.minw, k.code, k.flags, k.wv, k.conv, k.it, k.alpha, k.rule, (int64_t)(intptr_t)k.why};
        std::memcpy(keys + 11 * (size_t)i, v, sizeof v);
    }
}
// wave_cascade_once() of n shapes: the rule measured on the plain once-per-workgroup form of the cascade (kernel_choice.hpp)
void qt_wave_cascade_once(const KernelShape *shapes, int n, int32_t *once)
{
    for (int i = 0; i < n; ++i) once[i] = wave_cascade_once(shapes[i]) ? 1 : 0;
}
// wave_cascade_walk() of n shapes: 1 where the launch sets LadderArgs::wu_once -- the rule above, and the lengths the form serves since the waves
// below the top draw the next step's acceptance block in its wait
void qt_wave_cascade_walk(const KernelShape *shapes, int n, int32_t *walk)
{
    for (int i = 0; i < n; ++i) walk[i] = wave_cascade_walk(shapes[i]) ? 1 : 0;
}
// wave_cascade_mode() of n shapes: what the launch puts into LadderArgs::wu_once -- 0 the replay, 1 the walk on bounds the top rung's wave found, 2 the walk
// on bounds the waves below the top found, a pair each
void qt_wave_cascade_mode(const KernelShape *shapes, int n, int32_t *mode)
{
    for (int i = 0; i < n; ++i) mode[i] = wave_cascade_mode(shapes[i]);
}
int qt_kernel_shape_ints(void) { return (int)(sizeof(KernelShape) / sizeof(int)); }
// validate_params(), then the first phase of plan_host(): the QECMC_ERR_* code and message; accepted: the shape's static fields (the others 0)
int qt_plan_dims(const qecmc_params *p, int32_t *shape_ints, char *msg, int msg_cap)
{
    HostPlan hp;
    Refusal r = validate_params(p);
    if (!r.code) r = plan_dims(*p, hp);
    KernelShape s = {};
    if (!r.code) {
        s = kernel_shape(hp.args);
        s.gen_type = !hp.gen_type.empty();
    }
    return answer(r, s, shape_ints, msg, msg_cap);
}
// validate_params(), then plan_host(): accepted, the plan's shape, LDS bytes and persistent grid on a device of cu_count CUs
int qt_plan(const qecmc_params *p, int cu_count, int32_t *shape_ints, uint64_t *lds_bytes, uint32_t *grid, char *msg, int msg_cap)
{
    HostPlan hp;
    Refusal r = validate_params(p);
    if (!r.code) r = plan_host(*p, hp);
    if (!r.code) { *lds_bytes = hp.lds_bytes; *grid = queue_grid(hp, cu_count, p->flags); }
    return answer(r, hp.shape, shape_ints, msg, msg_cap);
}
// validate_params(), then plan_host(): the temperature ladder of an accepted block, as the kernels read it.  head[4] = acc_all_mask, swap_fast_ok,
// bias_f32ok, nq; inv_log2[kMaxNc] = swap_inv_log2; acc_thr[kMaxNc][4], acc_thr44[kMaxNc][4]; acc_top[nq + 1]; swap_thr[(Nc - 1)(nq + 1)] (either
// buffer may be null).  Returns the QECMC_ERR_* code with its message; QECMC_ERR_INVALID for too small a buffer
int qt_plan_ladder(const qecmc_params *p, uint32_t *head, float *inv_log2, uint32_t *acc_thr, uint64_t *acc_thr44, uint32_t *acc_top, int acc_top_cap,
                   uint64_t *swap_thr, int swap_thr_cap, char *msg, int msg_cap)
{
    HostPlan hp;
    Refusal r = validate_params(p);
    if (!r.code) r = plan_host(*p, hp);
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", r.msg.c_str());
    if (r.code) return r.code;
    const LadderArgs &a = hp.args;
    head[0] = a.acc_all_mask; head[1] = (uint32_t)a.swap_fast_ok; head[2] = a.bias_f32ok; head[3] = (uint32_t)a.nq;
    std::memcpy(inv_log2, a.swap_inv_log2, sizeof a.swap_inv_log2);
    std::memcpy(acc_thr, a.acc_thr, sizeof a.acc_thr);
    std::memcpy(acc_thr44, a.acc_thr44, sizeof a.acc_thr44);
    if ((acc_top && put(hp.acc_top, acc_top, acc_top_cap) < 0) || (swap_thr && put(hp.swap_thr, swap_thr, swap_thr_cap) < 0)) return QECMC_ERR_INVALID;
    return 0;
}
int qt_plan_key_equal(const qecmc_params *a, const qecmc_params *b)
{
    const qecmc_params ka = plan_key(*a), kb = plan_key(*b);
    return std::memcmp(&ka, &kb, sizeof ka) == 0;
}
// 1: the host plans of two accepted blocks are the same -- every table, lds_bytes, shape, queue fields, and args apart from the seed words
// (which a launch through the plan cache patches, see plan_key) --, 0: they differ, -1: a block is refused
int qt_plan_equal(const qecmc_params *pa, const qecmc_params *pb)
{
    HostPlan a, b;
    if (validate_params(pa).code || validate_params(pb).code || plan_host(*pa, a).code || plan_host(*pb, b).code) return -1;
    a.args.seed_lo = a.args.seed_hi = b.args.seed_lo = b.args.seed_hi = 0;
    return std::memcmp(&a.args, &b.args, sizeof a.args) == 0 && a.gen == b.gen && a.xyz_lut == b.xyz_lut && a.wu_desc == b.wu_desc && a.col_thr == b.col_thr &&
           a.lmask == b.lmask && a.acc_top == b.acc_top && a.gen_type == b.gen_type && a.phases == b.phases && a.bias == b.bias && a.lnb == b.lnb &&
           a.swap_thr == b.swap_thr && same_shape(a.shape, b.shape) && a.lds_bytes == b.lds_bytes && a.takes_queue == b.takes_queue &&
           a.queue_family == b.queue_family && a.queue_per_cu == b.queue_per_cu;
}
uint64_t qt_workspace_need(const qecmc_params *p, uint32_t grid, uint64_t N, int queue) { return workspace_need(*p, grid, N, queue != 0); }
// resume_conv_need(): the record and log bytes of a continued criterion run; resume_conv_check(): the QECMC_ERR_* code of the plan's refusal (0: accepted)
void qt_resume_conv_bytes(const qecmc_params *p, uint64_t N, uint64_t log_rows, uint64_t *record_bytes, uint64_t *log_bytes)
{
    const ResumeConvBytes need = resume_conv_need(*p, N, log_rows);
    *record_bytes = need.record;
    *log_bytes = need.log;
}
int qt_resume_conv_check(const qecmc_params *p, char *msg, int msg_cap)
{
    const Refusal r = resume_conv_check(*p);
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", r.msg.c_str());
    return r.code;
}
// rng_range_check(): the QECMC_ERR_* code with which the entry points that take step0 / prop0 / k0 refuse indices beyond the 48-bit Philox counter (0: accepted);
// resume != 0: prop0 is step0 * iters, as qecmc_pteq_resume_dev / qecmc_pteq_resume_conv_dev derive it (the argument is ignored)
int qt_rng_range_check(int resume, uint64_t step0, uint64_t nsteps, uint64_t prop0, uint64_t iters, char *msg, int msg_cap)
{
    const Refusal r = resume ? rng_range_check_resume("resume", step0, nsteps, iters) : rng_range_check("step", step0, nsteps, prop0, iters);
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", r.msg.c_str());
    return r.code;
}
// the shortest-chain statistics (qecmc_plan_set_shortest): what they refuse of a parameter block before a buffer is looked at, and the set workspace
int qt_shortest_check(const qecmc_params *p, char *msg, int msg_cap)
{
    Refusal r = validate_params(p);
    HostPlan hp;
    if (!r.code) r = plan_host(*p, hp);
    if (!r.code) r = shortest_check(*p, hp.shape);
    snprintf(msg, (size_t)msg_cap, "%s", r.msg.c_str());
    return r.code;
}
// LDS of an accepted plan's shortest-chain kernels: the bytes a launch asks for, the plan's plain figure, and -- scan = colour -- the dword at which the
// kernel keeps the kShortRows words of the statistics (0 otherwise); -1: the block is refused
int qt_shortest_lds(const qecmc_params *p, uint64_t *short_bytes, uint64_t *plain_bytes, uint32_t *colour_at, uint32_t *rows)
{
    HostPlan hp;
    if (validate_params(p).code || plan_host(*p, hp).code || shortest_check(*p, hp.shape).code) return -1;
    const LadderArgs &a = hp.args;
    *short_bytes = shortest_lds_bytes(a);
    *plain_bytes = hp.lds_bytes;
    *colour_at = p->scan == QECMC_SCAN_COLOUR ? colour_short_at(a.Nc, a.W, a.ncls, a.n_phases, a.n_gen, a.L, a.nq, a.swap_fast_ok != 0) : 0u;
    *rows = (uint32_t)kShortRows;
    return 0;
}
uint64_t qt_shortest_set_need(uint64_t N, uint64_t set_capacity) { return shortest_set_need(N, set_capacity); }
int qt_launch_takes_queue(uint32_t grid, uint64_t steps, int wants_states_or_stats) { return launch_takes_queue(grid, steps, wants_states_or_stats != 0); }
// the lift table of a code (syndrome_lift.hpp): uint32[cells][W + 1], W packed state words then the flag word (0: the cell is no check); the number of
// words, -1 for a (code, L) check_code_L() refuses.  qt_chains_from_syndromes: the host twin of qecmc_chains_from_syndromes -- lift_body(), the body the
// kernel runs, on a plain array; the QECMC_ERR_* code of the same host checks
int qt_lift_table(int code, int L, uint32_t *out, int cap)
{
    if (check_code_L(code, L).code) return -1;
    return put(lift::build_table(code, L).rows, out, cap);
}
int qt_chains_from_syndromes(int code, int L, uint64_t N, const uint8_t *defects, int descend, uint8_t *chains, uint8_t *status, int32_t *weight)
{
    if (!defects || !chains) return QECMC_ERR_INVALID;
    if (const Refusal r = check_code_L(code, L); r.code) return r.code;
    const lift::Table t = lift::build_table(code, L);
    if (t.rows.empty()) return QECMC_ERR_UNSUPPORTED;
    lift::chains_from_syndromes_host(t, N, defects, descend != 0, chains, status, weight);
    return 0;
}
// the class-move table of a code (corrections.hpp): uint32[ncls][ncls] bit masks over the logical kinds; the number of entries, 0 where the code's
// logical operators do not reach every class, -1 for a (code, L) check_code_L() refuses.  qt_corrections: the host twin of qecmc_corrections --
// correct_body(), the body the kernel runs, on a plain array; the QECMC_ERR_* code of the same host checks
int qt_class_moves(int code, int L, uint32_t *out, int cap)
{
    if (check_code_L(code, L).code) return -1;
    return put(correct::build_table(code, L).need, out, cap);
}
int qt_corrections(int code, int L, uint64_t N, uint32_t K, const uint8_t *candidates, const int32_t *target, int place, int descend, uint8_t *corrections,
                   int32_t *weight, int32_t *source, uint8_t *moved, uint8_t *status)
{
    if (!candidates || !target || !corrections || K == 0) return QECMC_ERR_INVALID;
    if (const Refusal r = check_code_L(code, L); r.code) return r.code;
    const correct::Table t = correct::build_table(code, L);
    if (t.need.empty()) return QECMC_ERR_UNSUPPORTED;
    correct::corrections_host(t, N, K, candidates, target, place != 0, descend != 0, corrections, weight, source, moved, status);
    return 0;
}
// the coset enumeration (enumerate.hpp).  qt_enumerate_info: rank, ncls, nq, the default chunk_bits, the LDS bytes and histogram copies of a
// workgroup -- the QECMC_ERR_* code of build_table()'s refusal; qt_enumerate_basis: the basis planes uint32[rank][2] (x, z), -1 where refused;
// qt_enumerate_shape: group, blocks and slice_bits of a launch; qt_coset_enumerate: the host twin of qecmc_coset_enumerate behind the same host checks
int qt_enumerate_info(int code, int L, int32_t *out6, char *msg, int msg_cap)
{
    const enumr::Table t = enumr::build_table(code, L);
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", t.refusal.msg.c_str());
    if (t.refusal.code) return t.refusal.code;
    int bits = 0;
    uint64_t count = 0;
    (void)enumr::resolve_range(t, bits, 0, count);
    const int32_t v[6] = {t.rank, t.ncls, t.nq, bits, (int32_t)t.carve.bytes, (int32_t)t.carve.copies};
    std::memcpy(out6, v, sizeof v);
    return 0;
}
int qt_enumerate_basis(int code, int L, uint32_t *out, int cap)
{
    const enumr::Table t = enumr::build_table(code, L);
    if (t.refusal.code) return -1;
    std::vector<uint32_t> v;
    for (int b = 0; b < t.rank; ++b) { v.push_back(t.gx[(size_t)b]); v.push_back(t.gz[(size_t)b]); }
    return put(v, out, cap);
}
void qt_enumerate_shape(int ncls, int chunk_bits, uint64_t N, uint32_t *group, uint32_t *blocks, int32_t *slice_bits)
{
    const enumr::Shape s = enumr::launch_shape(ncls, chunk_bits, N);
    *group = s.group; *blocks = s.blocks; *slice_bits = s.slice_bits;
}
int qt_coset_enumerate(int code, int L, uint64_t N, const uint8_t *chains, int chunk_bits, uint64_t chunk_first, uint64_t chunk_count, uint64_t *hist,
                       int32_t *cls)
{
    if (!chains || !hist) return QECMC_ERR_INVALID;
    const enumr::Table t = enumr::build_table(code, L);
    if (t.refusal.code) return t.refusal.code;
    if (const Refusal r = enumr::resolve_range(t, chunk_bits, chunk_first, chunk_count); r.code) return r.code;
    enumr::enumerate_host(t, N, chains, chunk_bits, chunk_first, chunk_count, hist, cls);
    return 0;
}
// the frontier sweep (class_sweep.hpp).  qt_class_sweep_info: width, ncls, nq, n_ops, rank, n_gen, the LDS bytes of a workgroup and kMaxWidth -- the
// QECMC_ERR_* code of build_plan()'s refusal (width and n_ops are the planner's even where it refuses the width); qt_class_sweep_ops: the op stream
// uint32[n_ops][4], -1 where refused; qt_class_sweep: the host twin of qecmc_class_sweep behind the same host checks
int qt_class_sweep_info(int code, int L, int32_t *out8, char *msg, int msg_cap)
{
    const sweep::Plan p = sweep::build_plan(code, L);
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", p.refusal.msg.c_str());
    const int32_t v[8] = {p.width, p.ncls, p.nq, p.n_ops, p.rank, p.n_gen, (int32_t)sweep::lds_carve(p.width).bytes, sweep::kMaxWidth};
    if (out8) std::memcpy(out8, v, sizeof v);
    return p.refusal.code;
}
int qt_class_sweep_ops(int code, int L, uint32_t *out, int cap)
{
    const sweep::Plan p = sweep::build_plan(code, L);
    if (p.refusal.code) return -1;
    return put(p.ops, out, cap);
}
int qt_class_sweep(int code, int L, uint64_t N, const uint8_t *chains, const double *w, double *z, int32_t *cls)
{
    if (!chains || !w || !z) return QECMC_ERR_INVALID;
    if (const Refusal r = sweep::check_weights(w); r.code) return r.code;
    const sweep::Plan p = sweep::build_plan(code, L);
    if (p.refusal.code) return p.refusal.code;
    sweep::sweep_host(p, N, chains, w, z, cls);
    return 0;
}
// the cut-set sweep (class_sweep_cut.hpp).  qt_class_sweep_cut_info: full_width, width, n_held, ncls, nq, n_ops, rank, n_gen, the LDS bytes of a
// workgroup, kMaxHeld, kCutMaxWidth, the lds_width the plan was built for -- the QECMC_ERR_* code of build_cut_plan()'s refusal;
// qt_class_sweep_cut_ops: the op stream, -1 where refused; qt_class_sweep_cut_held: the held generators' table indices int32[n_held] and packed words
// uint32[n_held][W] -> n_held, -1 where refused or too small a buffer; qt_class_sweep_cut_group: the syndromes of one launch; qt_class_sweep_cut: the
// host twin of qecmc_class_sweep_cut behind the same host checks
int qt_class_sweep_cut_info(int code, int L, int lds_width, int32_t *out12, char *msg, int msg_cap)
{
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", cp.plan.refusal.msg.c_str());
    const int32_t v[12] = {cp.full_width, cp.plan.width, cp.n_held, cp.plan.ncls, cp.plan.nq, cp.plan.n_ops, cp.plan.rank, cp.plan.n_gen,
                           (int32_t)sweep::lds_carve(cp.plan.width).bytes, sweep::kMaxHeld, sweep::kCutMaxWidth, cp.lds_width};
    if (out12) std::memcpy(out12, v, sizeof v);
    return cp.plan.refusal.code;
}
int qt_class_sweep_cut_ops(int code, int L, int lds_width, uint32_t *out, int cap)
{
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    if (cp.plan.refusal.code) return -1;
    return put(cp.plan.ops, out, cap);
}
int qt_class_sweep_cut_held(int code, int L, int lds_width, int32_t *index, uint32_t *words, int cap_words)
{
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    if (cp.plan.refusal.code || (int)cp.held_words.size() > cap_words) return -1;
    for (int j = 0; j < cp.n_held; ++j) index[j] = cp.held[(size_t)j];
    if (!cp.held_words.empty()) std::memcpy(words, cp.held_words.data(), cp.held_words.size() * sizeof(uint32_t));
    return cp.n_held;
}
uint32_t qt_class_sweep_cut_group(uint64_t N, int ncls, int n_held) { return sweep::cut_launch_group(N, ncls, n_held); }
int qt_class_sweep_cut(int code, int L, uint64_t N, const uint8_t *chains, const double *w, int lds_width, double *z, int32_t *cls)
{
    if (!chains || !w || !z) return QECMC_ERR_INVALID;
    if (const Refusal r = sweep::check_weights(w); r.code) return r.code;
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    if (cp.plan.refusal.code) return cp.plan.refusal.code;
    sweep::sweep_cut_host(cp, N, chains, w, z, cls);
    return 0;
}
// the tiled sweep (class_sweep_tiled.hpp).  qt_class_sweep_tiled_info: full_width, width, n_held, ncls, nq, n_ops, rank, n_gen, n_segments, state_bits,
// the hbm_width and tile_width the plan was built for, kMaxHeld, kTiledMaxWidth, the units of one pass and the threads of a workgroup -- the
// QECMC_ERR_* code of build_tiled_plan()'s refusal; qt_class_sweep_tiled_ops: the wide op stream uint32[n_ops][4]; qt_class_sweep_tiled_segments: the
// segment table uint32[n_segments][8] (op_first, op_count, tile, live, live_in, live_out, n_tiles, 0); qt_class_sweep_tiled_held: as the cut sweep's;
// qt_class_sweep_tiled: the host twin of qecmc_class_sweep_tiled behind the same host checks.  -1 where refused or too small a buffer
int qt_class_sweep_tiled_info(int code, int L, int hbm_width, int tile_width, int32_t *out16, char *msg, int msg_cap)
{
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", tp.plan.refusal.msg.c_str());
    const int32_t v[16] = {tp.full_width, tp.plan.width, tp.n_held, tp.plan.ncls, tp.plan.nq, tp.plan.n_ops, tp.plan.rank, tp.plan.n_gen, (int32_t)tp.segments.size(),
                           tp.state_bits, tp.hbm_width, tp.tile_width, sweep::kMaxHeld, sweep::kTiledMaxWidth,
                           tp.state_bits ? (int32_t)sweep::tiled_pass_units(tp.state_bits) : 0, tp.tile_width ? (int32_t)sweep::tiled_threads(tp.tile_width) : 0};
    if (out16) std::memcpy(out16, v, sizeof v);
    return tp.plan.refusal.code;
}
int qt_class_sweep_tiled_ops(int code, int L, int hbm_width, int tile_width, uint32_t *out, int cap)
{
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (tp.plan.refusal.code) return -1;
    return put(tp.ops, out, cap);
}
int qt_class_sweep_tiled_segments(int code, int L, int hbm_width, int tile_width, uint32_t *out, int cap)
{
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (tp.plan.refusal.code) return -1;
    std::vector<uint32_t> v;
    for (const sweep::Segment &sg : tp.segments) {
        const uint32_t w[sweep::kSegmentWords] = {sg.op_first, sg.op_count, sg.tile, sg.live, sg.live_in, sg.live_out, sg.n_tiles, 0u};
        v.insert(v.end(), w, w + sweep::kSegmentWords);
    }
    return put(v, out, cap);
}
int qt_class_sweep_tiled_held(int code, int L, int hbm_width, int tile_width, int32_t *index, uint32_t *words, int cap_words)
{
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (tp.plan.refusal.code || (int)tp.held_words.size() > cap_words) return -1;
    for (int j = 0; j < tp.n_held; ++j) index[j] = tp.held[(size_t)j];
    if (!tp.held_words.empty()) std::memcpy(words, tp.held_words.data(), tp.held_words.size() * sizeof(uint32_t));
    return tp.n_held;
}
int qt_class_sweep_tiled(int code, int L, uint64_t N, const uint8_t *chains, const double *w, int hbm_width, int tile_width, double *z, int32_t *cls)
{
    if (!chains || !w || !z) return QECMC_ERR_INVALID;
    if (const Refusal r = sweep::check_weights(w); r.code) return r.code;
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (tp.plan.refusal.code) return tp.plan.refusal.code;
    sweep::sweep_tiled_host(tp, N, chains, w, z, cls);
    return 0;
}
// the sweeps under site weights (class_sweep_site.hpp): the host twins of qecmc_class_sweep_site, _cut_site and _tiled_site behind the same host checks,
// in the same order -- the QECMC_ERR_* code of the refusal, its message in msg (nullable)
static int site_answer(const Refusal &r, char *msg, int msg_cap)
{
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%s", r.msg.c_str());
    return r.code;
}
static Refusal site_checks(uint64_t N, const double *wq, uint64_t wq_rows, int nq, const std::vector<uint32_t> &ops)
{
    if (const Refusal r = sweep::check_site_rows(N, wq_rows); r.code) return r;
    return N ? sweep::check_site_weights(wq, wq_rows, nq, sweep::closed_qubits(ops, nq)) : Refusal{};
}
int qt_class_sweep_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, double *z, int32_t *cls, char *msg, int msg_cap)
{
    if (!chains || !wq || !z) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_sweep_site: NULL buffer"), msg, msg_cap);
    const sweep::Plan p = sweep::build_plan(code, L);
    if (p.refusal.code) return site_answer(p.refusal, msg, msg_cap);
    if (const Refusal r = site_checks(N, wq, wq_rows, p.nq, p.ops); r.code) return site_answer(r, msg, msg_cap);
    sweep::sweep_site_host(p, N, chains, wq, wq_rows, z, cls);
    return site_answer({}, msg, msg_cap);
}
int qt_class_sweep_cut_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int lds_width, double *z, int32_t *cls, char *msg,
                            int msg_cap)
{
    if (!chains || !wq || !z) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_sweep_cut_site: NULL buffer"), msg, msg_cap);
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    if (cp.plan.refusal.code) return site_answer(cp.plan.refusal, msg, msg_cap);
    if (const Refusal r = site_checks(N, wq, wq_rows, cp.plan.nq, cp.plan.ops); r.code) return site_answer(r, msg, msg_cap);
    sweep::sweep_cut_site_host(cp, N, chains, wq, wq_rows, z, cls);
    return site_answer({}, msg, msg_cap);
}
int qt_class_sweep_tiled_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int hbm_width, int tile_width, double *z, int32_t *cls,
                              char *msg, int msg_cap)
{
    if (!chains || !wq || !z) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_sweep_tiled_site: NULL buffer"), msg, msg_cap);
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (tp.plan.refusal.code) return site_answer(tp.plan.refusal, msg, msg_cap);
    if (const Refusal r = site_checks(N, wq, wq_rows, tp.plan.nq, tp.ops); r.code) return site_answer(r, msg, msg_cap);
    sweep::sweep_tiled_site_host(tp, N, chains, wq, wq_rows, z, cls);
    return site_answer({}, msg, msg_cap);
}
// the (min, +, count) sweep (class_minplus.hpp).  qt_class_minplus: the host twin of qecmc_class_minplus behind the same host checks, in the same
// order -- the QECMC_ERR_* code of the refusal, its message in msg (nullable); qt_minplus_combine: mp_combine on two packed entries, and through out3
// (nullable) kSat, the bits of a count and the largest cost
int qt_class_minplus(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t *cost, int lds_width, uint32_t *cost_out, uint64_t *count_out, int32_t *cls,
                     char *msg, int msg_cap)
{
    if (!chains || !cost || !cost_out || !count_out) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus: NULL buffer"), msg, msg_cap);
    if (N > 0xFFFFFFFFull) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus: N=%llu syndromes exceed 32 bits", (unsigned long long)N), msg, msg_cap);
    if (const Refusal r = minplus::check_costs(cost); r.code) return site_answer(r, msg, msg_cap);
    const sweep::CutPlan cp = minplus::build_minplus_plan(code, L, lds_width);
    if (cp.plan.refusal.code) return site_answer(cp.plan.refusal, msg, msg_cap);
    minplus::minplus_cut_host(cp, N, chains, cost, cost_out, count_out, cls);
    return site_answer({}, msg, msg_cap);
}
uint64_t qt_minplus_combine(uint64_t a, uint64_t b, uint64_t *out3)
{
    if (out3) { out3[0] = minplus::kSat; out3[1] = (uint64_t)minplus::kCountBits; out3[2] = minplus::kMaxCost; }
    return minplus::mp_combine(a, b);
}
// the traceback (class_minplus_trace.hpp).  qt_class_minplus_chains: the host twin of qecmc_class_minplus_chains behind the same host checks, in the
// same order; qt_class_minplus_trace_plan: forget_gen int32[n_forget] and forget_words uint32[n_forget][W] -> n_forget, -1 where refused or too small
// a buffer, and through out4 (nullable) n_forget, words_per_forget, W and the bytes of one pair's decisions; qt_class_minplus_trace_group: the
// syndromes of one launch, and through workspace (nullable) the bound on a group's decision words
int qt_class_minplus_chains(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t *cost, int lds_width, uint8_t *chain_out, uint32_t *cost_out,
                            uint64_t *count_out, int32_t *cls, char *msg, int msg_cap)
{
    if (!chains || !cost || !chain_out) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_chains: NULL buffer"), msg, msg_cap);
    if (N > 0xFFFFFFFFull) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_chains: N=%llu syndromes exceed 32 bits", (unsigned long long)N), msg, msg_cap);
    if (const Refusal r = minplus::check_chain_costs(cost); r.code) return site_answer(r, msg, msg_cap);
    const minplus::TracePlan tp = minplus::build_trace_plan(code, L, lds_width);
    if (tp.cut.plan.refusal.code) return site_answer(tp.cut.plan.refusal, msg, msg_cap);
    minplus::minplus_trace_host(tp, N, chains, cost, chain_out, cost_out, count_out, cls);
    return site_answer({}, msg, msg_cap);
}
int qt_class_minplus_trace_plan(int code, int L, int lds_width, int32_t *forget_gen, uint32_t *forget_words, int cap_words, int32_t *out4)
{
    const minplus::TracePlan tp = minplus::build_trace_plan(code, L, lds_width);
    if (tp.cut.plan.refusal.code || (int)tp.forget_words.size() > cap_words) return -1;
    for (int i = 0; i < tp.n_forget; ++i) forget_gen[i] = tp.forget_gen[(size_t)i];
    if (!tp.forget_words.empty()) std::memcpy(forget_words, tp.forget_words.data(), tp.forget_words.size() * sizeof(uint32_t));
    if (out4) { out4[0] = tp.n_forget; out4[1] = tp.words_per_forget; out4[2] = tp.cut.plan.W; out4[3] = (int32_t)minplus::trace_bytes_per_pair(tp); }
    return tp.n_forget;
}
uint32_t qt_class_minplus_trace_group(uint64_t N, int ncls, int n_held, uint64_t bytes_per_pair, uint64_t *workspace)
{
    if (workspace) *workspace = minplus::kTraceWorkspaceBytes;
    return minplus::trace_launch_group(N, ncls, n_held, bytes_per_pair);
}
// the (min, +) sweep and its traceback under site costs (class_minplus_site.hpp): the host twins of qecmc_class_minplus_site and
// qecmc_class_minplus_chains_site behind the same host checks, in the same order -- the QECMC_ERR_* code of the refusal, its message in msg (nullable);
// qt_site_cost_words: rows of cq as the words host and device read, out uint32[rows][nq]
int qt_class_minplus_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int lds_width, uint32_t *cost_out, uint64_t *count_out,
                          int32_t *cls, char *msg, int msg_cap)
{
    if (!chains || !cq || !cost_out || !count_out) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_site: NULL buffer"), msg, msg_cap);
    if (N > 0xFFFFFFFFull) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_site: N=%llu syndromes exceed 32 bits", (unsigned long long)N), msg, msg_cap);
    const sweep::CutPlan cp = minplus::build_minplus_site_plan(code, L, lds_width);
    if (cp.plan.refusal.code) return site_answer(cp.plan.refusal, msg, msg_cap);
    if (const Refusal r = minplus::check_cost_rows("qecmc_class_minplus_site", N, cq_rows); r.code) return site_answer(r, msg, msg_cap);
    minplus::minplus_cut_site_host(cp, N, chains, cq, cq_rows, cost_out, count_out, cls);
    return site_answer({}, msg, msg_cap);
}
int qt_class_minplus_chains_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int lds_width, uint8_t *chain_out, uint32_t *cost_out,
                                 uint64_t *count_out, int32_t *cls, char *msg, int msg_cap)
{
    if (!chains || !cq || !chain_out) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_chains_site: NULL buffer"), msg, msg_cap);
    if (N > 0xFFFFFFFFull)
        return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_chains_site: N=%llu syndromes exceed 32 bits", (unsigned long long)N), msg, msg_cap);
    const minplus::TracePlan tp = minplus::build_trace_site_plan(code, L, lds_width);
    if (tp.cut.plan.refusal.code) return site_answer(tp.cut.plan.refusal, msg, msg_cap);
    if (const Refusal r = minplus::check_cost_rows("qecmc_class_minplus_chains_site", N, cq_rows); r.code) return site_answer(r, msg, msg_cap);
    minplus::minplus_trace_site_host(tp, N, chains, cq, cq_rows, chain_out, cost_out, count_out, cls);
    return site_answer({}, msg, msg_cap);
}
void qt_site_cost_words(const uint8_t *cq, uint64_t rows, int nq, uint32_t *out) { minplus::site_cost_words(cq, rows, nq, out); }
// the exact chain sampler (class_sample.hpp).  qt_class_sample: the host twin of qecmc_class_sample (w given) and qecmc_class_sample_site (w NULL) behind
// the same host checks, in the same order -- the QECMC_ERR_* code of the refusal, its message in msg (nullable); qt_class_sample_plan: forget_gen
// int32[n_forget] and forget_words uint32[n_forget][W] (both nullable) -> n_forget, -1 where refused or too small a buffer, and through out6 (nullable)
// n_forget, W, width, n_held, the workspace bound and the bytes of one job's record; qt_class_sample_group: syndromes, k_chunk and jobs of one launch;
// qt_class_sample_u53: the uniform of one Philox address
int qt_class_sample(int code, int L, uint64_t N, const uint8_t *chains, const double *w, const double *wq, uint64_t wq_rows, int lds_width, uint64_t K, uint64_t seed,
                    uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out, char *msg, int msg_cap)
{
    const char *name = w ? "qecmc_class_sample" : "qecmc_class_sample_site";
    if (!chains || (!w && !wq) || !chain_out || !z_out || (mode == 1 && !class_out)) return site_answer(refuse_params(QECMC_ERR_INVALID, "%s: NULL buffer", name), msg, msg_cap);
    if (const Refusal r = sample::check_sample_args(name, N, K, first_syndrome, mode); r.code) return site_answer(r, msg, msg_cap);
    if (w)
        if (const Refusal r = sample::check_sample_weights(name, w); r.code) return site_answer(r, msg, msg_cap);
    const sample::SamplePlan sp = sample::build_sample_plan(code, L, lds_width, name);
    if (sp.cut.plan.refusal.code) return site_answer(sp.cut.plan.refusal, msg, msg_cap);
    if (!w)
        if (const Refusal r = sample::check_sample_site(name, N, wq, wq_rows, sp.cut.plan); r.code) return site_answer(r, msg, msg_cap);
    return site_answer(sample::sample_host(sp, name, N, chains, w, wq, wq_rows, K, seed, first_syndrome, mode, chain_out, class_out, z_out), msg, msg_cap);
}
int qt_class_sample_plan(int code, int L, int lds_width, int32_t *forget_gen, uint32_t *forget_words, int cap_words, uint64_t *out6)
{
    const sample::SamplePlan sp = sample::build_sample_plan(code, L, lds_width);
    if (sp.cut.plan.refusal.code || (forget_words && (int)sp.forget_words.size() > cap_words)) return -1;
    if (forget_gen)
        for (int i = 0; i < sp.n_forget; ++i) forget_gen[i] = sp.forget_gen[(size_t)i];
    if (forget_words && !sp.forget_words.empty()) std::memcpy(forget_words, sp.forget_words.data(), sp.forget_words.size() * sizeof(uint32_t));
    if (out6) {
        out6[0] = (uint64_t)sp.n_forget; out6[1] = (uint64_t)sp.cut.plan.W; out6[2] = (uint64_t)sp.cut.plan.width; out6[3] = (uint64_t)sp.cut.n_held;
        out6[4] = sample::kSampleWorkspaceBytes; out6[5] = sample::sample_bytes_per_job(sp);
    }
    return sp.n_forget;
}
void qt_class_sample_group(uint64_t N, int ncls, int n_held, uint64_t K, uint64_t bytes_per_job, uint32_t *out3)
{
    const sample::LaunchGroup g = sample::sample_launch_group(N, ncls, n_held, K, bytes_per_job);
    out3[0] = g.syndromes; out3[1] = g.k_chunk; out3[2] = g.jobs;
}
double qt_class_sample_u53(uint64_t k, uint32_t block, uint32_t j, uint32_t syndrome, uint32_t stream, uint64_t seed) { return sample::draw_u53(k, block, j, syndrome, stream, seed); }
double qt_class_sample_floor() { return sample::kSampleFloor; }
// qt_class_sample_record: what one job of the twin walks, for the tests that compute the law THE RULE assigns without draws.  One syndrome (chain
// uint8[nq]; w[4], or one table row wq double[nq][4] where w is NULL), class cls, held assignment h -> pairs double[n_forget][2^(width - 1)][2] as (on, s)
// -- record_one's, zeros at dead f --, the unfolded partials of the class double[2^n_held] and z double[ncls] as sample_host forms them, the start
// chain cut_representative(rep_cls, h) as uint32[W], and word 0 of every op uint32[n_ops].  No check of z: the caller judges.  -> n_ops, -1 where a
// buffer is NULL or too small, the class or h out of range, or the plan or the weights refused
int qt_class_sample_record(int code, int L, const uint8_t *chain, const double *w, const double *wq, int lds_width, int cls, uint32_t h, double *pairs_out, uint64_t pairs_cap,
                           double *partials_out, double *z_out, uint32_t *rep_out, uint32_t *ops_out, int ops_cap)
{
    const char *name = w ? "qecmc_class_sample" : "qecmc_class_sample_site";
    if (!chain || (!w && !wq) || !pairs_out || !partials_out || !z_out || !rep_out || !ops_out) return -1;
    if (w && sample::check_sample_weights(name, w).code) return -1;
    const sample::SamplePlan sp = sample::build_sample_plan(code, L, lds_width, name);
    const sweep::CutPlan &cp = sp.cut;
    const sweep::Plan &p = cp.plan;
    if (p.refusal.code || (!w && sample::check_sample_site(name, 1, wq, 1, p).code)) return -1;
    const uint32_t n_h = 1u << cp.n_held;
    const uint64_t pairs = sample::sample_pairs_per_job(sp.n_forget, p.width);
    if (cls < 0 || cls >= p.ncls || h >= n_h || pairs > pairs_cap || p.n_ops > ops_cap) return -1;
    sweep::Plan unscaled = p;
    unscaled.scale = 1.0;
    std::vector<double> wxz(w ? 4u : (size_t)p.nq * 4u), A((size_t)1 << p.width), fold((size_t)n_h);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W);
    if (w) sweep::weights_xz(w, wxz.data());
    else sweep::site_rows_xz(wq, 1, p.nq, wxz.data());
    sweep::class_representatives(p, chain, reps.data());
    for (int c = 0; c < p.ncls; ++c) {
        for (uint32_t i = 0; i < n_h; ++i) {
            sweep::cut_representative(cp, &reps[(size_t)c * p.W], i, rep.data());
            fold[i] = w ? sweep::sweep_one(unscaled, rep.data(), wxz.data(), A.data()) : sweep::sweep_one_site(unscaled, rep.data(), wxz.data(), A.data());
        }
        if (c == cls) std::memcpy(partials_out, fold.data(), (size_t)n_h * sizeof(double));
        z_out[c] = sweep::cut_reduce(fold.data(), cp.n_held, p.scale);
    }
    sweep::cut_representative(cp, &reps[(size_t)cls * p.W], h, rep.data());
    std::vector<sample::PairRecord> R((size_t)pairs, sample::PairRecord{0.0, 0.0});
    sample::record_one(sp, rep.data(), sample::Factors{wxz.data(), w ? 0u : 4u}, A.data(), R.data());
    std::memcpy(pairs_out, R.data(), (size_t)pairs * sizeof(sample::PairRecord));
    std::memcpy(rep_out, rep.data(), (size_t)p.W * sizeof(uint32_t));
    for (int o = 0; o < p.n_ops; ++o) ops_out[o] = p.ops[(size_t)o * sweep::kOpWords];
    return p.n_ops;
}
// the exact marginals (class_marginal.hpp).  qt_class_marginals: the host twin of qecmc_class_marginals (w given) and qecmc_class_marginals_site (w NULL)
// behind the same host checks, in the same order -- the QECMC_ERR_* code of the refusal, its message in msg (nullable); qt_class_marginals_plan: through
// out8 width, n_held, n_close, the bytes of one job's forward record, the workspace bound, the bound on a group's M_h, n_ops and nq, and through close_qubit
// (nullable, cap entries) the qubit of every CLOSE -> n_close, -1 where refused or too small a buffer; qt_class_marginals_group: syndromes and jobs of one launch
int qt_class_marginals(int code, int L, uint64_t N, const uint8_t *chains, const double *w, const double *wq, uint64_t wq_rows, int lds_width, double *weights_out,
                       double *z_out, int32_t *class_out, char *msg, int msg_cap)
{
    const char *name = w ? "qecmc_class_marginals" : "qecmc_class_marginals_site";
    if (!chains || (!w && !wq) || !weights_out || !z_out) return site_answer(refuse_params(QECMC_ERR_INVALID, "%s: NULL buffer", name), msg, msg_cap);
    if (const Refusal r = marginal::check_marginal_args(name, N); r.code) return site_answer(r, msg, msg_cap);
    if (w)
        if (const Refusal r = marginal::check_marginal_weights(name, w); r.code) return site_answer(r, msg, msg_cap);
    const marginal::MarginalPlan mp = marginal::build_marginal_plan(code, L, lds_width, name);
    if (mp.cut.plan.refusal.code) return site_answer(mp.cut.plan.refusal, msg, msg_cap);
    if (!w)
        if (const Refusal r = marginal::check_marginal_site(name, N, wq, wq_rows, mp.cut.plan); r.code) return site_answer(r, msg, msg_cap);
    marginal::marginal_host(mp, N, chains, w, wq, wq_rows, weights_out, z_out, class_out);
    return site_answer({}, msg, msg_cap);
}
int qt_class_marginals_plan(int code, int L, int lds_width, uint32_t *close_qubit, int cap, uint64_t *out8)
{
    const marginal::MarginalPlan mp = marginal::build_marginal_plan(code, L, lds_width);
    if (mp.cut.plan.refusal.code || (close_qubit && mp.n_close > cap)) return -1;
    if (close_qubit)
        for (int i = 0; i < mp.n_close; ++i) close_qubit[i] = mp.close_qubit[(size_t)i];
    if (out8) {
        out8[0] = (uint64_t)mp.cut.plan.width; out8[1] = (uint64_t)mp.cut.n_held; out8[2] = (uint64_t)mp.n_close; out8[3] = marginal::marginal_bytes_per_job(mp);
        out8[4] = marginal::kMarginalWorkspaceBytes; out8[5] = marginal::kMarginalFoldBytes; out8[6] = (uint64_t)mp.cut.plan.n_ops; out8[7] = (uint64_t)mp.cut.plan.nq;
    }
    return mp.n_close;
}
void qt_class_marginals_group(uint64_t N, int ncls, int n_held, int n_close, uint64_t bytes_per_job, uint32_t *out2)
{
    const marginal::LaunchGroup g = marginal::marginal_launch_group(N, ncls, n_held, n_close, bytes_per_job);
    out2[0] = g.syndromes; out2[1] = g.jobs;
}
// the (min, +) sweep on the tiled plans (class_minplus_tiled.hpp): the host twins of qecmc_class_minplus_tiled and qecmc_class_minplus_tiled_site behind
// the same host checks, in the same order -- the QECMC_ERR_* code of the refusal, its message in msg (nullable)
int qt_class_minplus_tiled(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t *cost, int hbm_width, int tile_width, uint32_t *cost_out, uint64_t *count_out,
                           int32_t *cls, char *msg, int msg_cap)
{
    if (!chains || !cost || !cost_out || !count_out) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled: NULL buffer"), msg, msg_cap);
    if (N > 0xFFFFFFFFull) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled: N=%llu syndromes exceed 32 bits", (unsigned long long)N), msg, msg_cap);
    if (const Refusal r = minplus::check_tiled_costs(cost); r.code) return site_answer(r, msg, msg_cap);
    const sweep::TiledPlan tp = minplus::build_minplus_tiled_plan(code, L, hbm_width, tile_width, "qecmc_class_minplus_tiled");
    if (tp.plan.refusal.code) return site_answer(tp.plan.refusal, msg, msg_cap);
    if (const Refusal r = minplus::check_tiled_cost_range(tp.plan, cost); r.code) return site_answer(r, msg, msg_cap);
    minplus::minplus_tiled_host(tp, N, chains, cost, cost_out, count_out, cls);
    return site_answer({}, msg, msg_cap);
}
int qt_class_minplus_tiled_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int hbm_width, int tile_width, uint32_t *cost_out,
                                uint64_t *count_out, int32_t *cls, char *msg, int msg_cap)
{
    if (!chains || !cq || !cost_out || !count_out) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled_site: NULL buffer"), msg, msg_cap);
    if (N > 0xFFFFFFFFull)
        return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled_site: N=%llu syndromes exceed 32 bits", (unsigned long long)N), msg, msg_cap);
    const sweep::TiledPlan tp = minplus::build_minplus_tiled_plan(code, L, hbm_width, tile_width, "qecmc_class_minplus_tiled_site");
    if (tp.plan.refusal.code) return site_answer(tp.plan.refusal, msg, msg_cap);
    if (const Refusal r = minplus::check_cost_rows("qecmc_class_minplus_tiled_site", N, cq_rows); r.code) return site_answer(r, msg, msg_cap);
    if (N > 0)
        if (const Refusal r = minplus::check_tiled_cost_rows_range(cq, cq_rows, tp.plan.nq, sweep::closed_qubits(tp.ops, tp.plan.nq)); r.code) return site_answer(r, msg, msg_cap);
    minplus::minplus_tiled_site_host(tp, N, chains, cq, cq_rows, cost_out, count_out, cls);
    return site_answer({}, msg, msg_cap);
}
// the traceback on the tiled plans (class_minplus_tiled_trace.hpp).  qt_class_minplus_tiled_chains (cost given) / ..._site (cq given): the host twins of
// qecmc_class_minplus_tiled_chains and ..._chains_site behind the same host checks, in the same order -- the QECMC_ERR_* code of the refusal, its message
// in msg (nullable); qt_class_minplus_tiled_trace_plan: forget_gen int32[n_forget], forget_words uint32[n_forget][W], forget_tile uint32[n_forget][4] and
// seg_forget uint32[n_segments] (all nullable) under a decision block of `cap` bytes (0: the library's) -> n_forget, -1 where refused (the message in msg)
// or too small a buffer (cap_forget rows), and through out8 (nullable) n_forget, words_per_tile, W, bytes_per_pair, the library's cap, state_bits,
// n_segments and n_held; qt_class_minplus_tiled_trace_pass: the pairs of one trace pass
static int tiled_chains_answer(const char *name, int code, int L, uint64_t N, const uint8_t *chains, const uint32_t *cost, const uint8_t *cq, uint64_t cq_rows, int hbm_width,
                               int tile_width, uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out, int32_t *cls, char *msg, int msg_cap)
{
    if (!chains || (!cost && !cq) || !chain_out) return site_answer(refuse_params(QECMC_ERR_INVALID, "%s: NULL buffer", name), msg, msg_cap);
    if (N > 0xFFFFFFFFull) return site_answer(refuse_params(QECMC_ERR_INVALID, "%s: N=%llu syndromes exceed 32 bits", name, (unsigned long long)N), msg, msg_cap);
    if (cost)
        if (const Refusal r = minplus::check_tiled_chain_costs(nullptr, cost); r.code) return site_answer(r, msg, msg_cap);
    const minplus::TiledTracePlan ttp = minplus::build_tiled_trace_plan(code, L, hbm_width, tile_width, name);
    const sweep::TiledPlan &tp = ttp.tiled;
    if (tp.plan.refusal.code) return site_answer(tp.plan.refusal, msg, msg_cap);
    if (cost) {
        if (const Refusal r = minplus::check_tiled_chain_costs(&tp.plan, cost); r.code) return site_answer(r, msg, msg_cap);
        minplus::minplus_tiled_trace_host(ttp, N, chains, cost, chain_out, cost_out, count_out, cls);
    } else {
        if (const Refusal r = minplus::check_cost_rows(name, N, cq_rows); r.code) return site_answer(r, msg, msg_cap);
        if (N > 0)
            if (const Refusal r = minplus::check_tiled_chain_cost_rows_range(cq, cq_rows, tp.plan.nq, sweep::closed_qubits(tp.ops, tp.plan.nq)); r.code)
                return site_answer(r, msg, msg_cap);
        minplus::minplus_tiled_trace_site_host(ttp, N, chains, cq, cq_rows, chain_out, cost_out, count_out, cls);
    }
    return site_answer({}, msg, msg_cap);
}
int qt_class_minplus_tiled_chains(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t *cost, int hbm_width, int tile_width, uint8_t *chain_out,
                                  uint32_t *cost_out, uint64_t *count_out, int32_t *cls, char *msg, int msg_cap)
{
    if (!cost) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled_chains: NULL buffer"), msg, msg_cap);
    return tiled_chains_answer("qecmc_class_minplus_tiled_chains", code, L, N, chains, cost, nullptr, 0, hbm_width, tile_width, chain_out, cost_out, count_out, cls, msg, msg_cap);
}
int qt_class_minplus_tiled_chains_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int hbm_width, int tile_width,
                                       uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out, int32_t *cls, char *msg, int msg_cap)
{
    if (!cq) return site_answer(refuse_params(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled_chains_site: NULL buffer"), msg, msg_cap);
    return tiled_chains_answer("qecmc_class_minplus_tiled_chains_site", code, L, N, chains, nullptr, cq, cq_rows, hbm_width, tile_width, chain_out, cost_out, count_out, cls,
                               msg, msg_cap);
}
int qt_class_minplus_tiled_trace_plan(int code, int L, int hbm_width, int tile_width, uint64_t cap, int32_t *forget_gen, uint32_t *forget_words, uint32_t *forget_tile,
                                      uint32_t *seg_forget, int cap_forget, uint64_t *out8, char *msg, int msg_cap)
{
    const minplus::TiledTracePlan ttp =
        minplus::build_tiled_trace_plan(code, L, hbm_width, tile_width, "qecmc_class_minplus_tiled_chains", cap ? cap : minplus::kTiledTraceWorkspaceBytes);
    const sweep::TiledPlan &tp = ttp.tiled;
    if (tp.plan.refusal.code) { site_answer(tp.plan.refusal, msg, msg_cap); return -1; }
    if ((forget_gen || forget_words || forget_tile) && ttp.n_forget > cap_forget) return -1;
    if (seg_forget && (int)tp.segments.size() > cap_forget) return -1;
    if (forget_gen)
        for (int i = 0; i < ttp.n_forget; ++i) forget_gen[i] = ttp.forget_gen[(size_t)i];
    if (forget_words) std::memcpy(forget_words, ttp.forget_words.data(), ttp.forget_words.size() * sizeof(uint32_t));
    if (forget_tile) std::memcpy(forget_tile, ttp.forget_tile.data(), ttp.forget_tile.size() * sizeof(uint32_t));
    if (seg_forget) std::memcpy(seg_forget, ttp.seg_forget.data(), ttp.seg_forget.size() * sizeof(uint32_t));
    if (out8) {
        out8[0] = (uint64_t)ttp.n_forget; out8[1] = (uint64_t)ttp.words_per_tile; out8[2] = (uint64_t)tp.plan.W; out8[3] = minplus::tiled_trace_bytes_per_pair(ttp);
        out8[4] = minplus::kTiledTraceWorkspaceBytes; out8[5] = (uint64_t)tp.state_bits; out8[6] = (uint64_t)tp.segments.size(); out8[7] = (uint64_t)tp.n_held;
    }
    return ttp.n_forget;
}
uint32_t qt_class_minplus_tiled_trace_pass(int state_bits, uint64_t bytes_per_pair, uint64_t pairs_left, uint64_t cap)
{
    return minplus::tiled_trace_pass_pairs(state_bits, bytes_per_pair, pairs_left, cap ? cap : minplus::kTiledTraceWorkspaceBytes);
}
// the exact sampler on the tiled plans (class_sample_tiled.hpp).  qt_class_sample_tiled: the host twin of qecmc_class_sample_tiled (w given) and
// qecmc_class_sample_tiled_site (w NULL) behind the same host checks, in the same order -- the QECMC_ERR_* code of the refusal, its message in msg
// (nullable); qt_class_sample_tiled_plan: forget_gen int32[n_forget], forget_words uint32[n_forget][W], forget_tile uint32[n_forget][4], pair_off
// uint64[n_forget + 1] and seg_forget uint32[n_segments] (all nullable) under a record block of `cap` bytes (0: the library's default) -> n_forget, -1
// where refused (the message in msg) or too small a buffer (cap_forget rows); through out8 (nullable, written for a plan refused for the cap alone as
// well) n_forget, bytes_per_job, W, the default cap, the largest cap, state_bits, n_segments and n_held; qt_class_sample_tiled_pass: the jobs of one
// record pass
int qt_class_sample_tiled(int code, int L, uint64_t N, const uint8_t *chains, const double *w, const double *wq, uint64_t wq_rows, int hbm_width, int tile_width,
                          uint64_t record_bytes, uint64_t K, uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out, char *msg,
                          int msg_cap)
{
    const char *name = w ? "qecmc_class_sample_tiled" : "qecmc_class_sample_tiled_site";
    if (!chains || (!w && !wq) || !chain_out || !z_out || (mode == 1 && !class_out)) return site_answer(refuse_params(QECMC_ERR_INVALID, "%s: NULL buffer", name), msg, msg_cap);
    if (const Refusal r = sample::check_sample_args(name, N, K, first_syndrome, mode); r.code) return site_answer(r, msg, msg_cap);
    if (w)
        if (const Refusal r = sample::check_sample_weights(name, w); r.code) return site_answer(r, msg, msg_cap);
    uint64_t cap = 0;
    if (const Refusal r = sample::check_record_bytes(name, record_bytes, &cap); r.code) return site_answer(r, msg, msg_cap);
    const sample::TiledSamplePlan tsp = sample::build_tiled_sample_plan(code, L, hbm_width, tile_width, name, cap);
    if (tsp.tiled.plan.refusal.code) return site_answer(tsp.tiled.plan.refusal, msg, msg_cap);
    if (!w)
        if (const Refusal r = sample::check_sample_tiled_site(name, N, wq, wq_rows, tsp.tiled); r.code) return site_answer(r, msg, msg_cap);
    return site_answer(sample::sample_tiled_host(tsp, name, N, chains, w, wq, wq_rows, K, seed, first_syndrome, mode, chain_out, class_out, z_out), msg, msg_cap);
}
int qt_class_sample_tiled_plan(int code, int L, int hbm_width, int tile_width, uint64_t cap, int32_t *forget_gen, uint32_t *forget_words, uint32_t *forget_tile,
                               uint64_t *pair_off, uint32_t *seg_forget, int cap_forget, uint64_t *out8, char *msg, int msg_cap)
{
    const sample::TiledSamplePlan tsp =
        sample::build_tiled_sample_plan(code, L, hbm_width, tile_width, "qecmc_class_sample_tiled", cap ? cap : sample::kTiledSampleRecordBytes);
    const sweep::TiledPlan &tp = tsp.tiled;
    if (out8 && tsp.n_forget > 0) {
        out8[0] = (uint64_t)tsp.n_forget; out8[1] = sample::tiled_sample_bytes_per_job(tsp); out8[2] = (uint64_t)tp.plan.W; out8[3] = sample::kTiledSampleRecordBytes;
        out8[4] = sample::kTiledSampleRecordBytesMax; out8[5] = (uint64_t)tp.state_bits; out8[6] = (uint64_t)tp.segments.size(); out8[7] = (uint64_t)tp.n_held;
    }
    if (tp.plan.refusal.code) { site_answer(tp.plan.refusal, msg, msg_cap); return -1; }
    if ((forget_gen || forget_words || forget_tile || pair_off) && tsp.n_forget > cap_forget) return -1;
    if (seg_forget && (int)tp.segments.size() > cap_forget) return -1;
    if (forget_gen)
        for (int i = 0; i < tsp.n_forget; ++i) forget_gen[i] = tsp.forget_gen[(size_t)i];
    if (forget_words) std::memcpy(forget_words, tsp.forget_words.data(), tsp.forget_words.size() * sizeof(uint32_t));
    if (forget_tile) std::memcpy(forget_tile, tsp.forget_tile.data(), tsp.forget_tile.size() * sizeof(uint32_t));
    if (pair_off) std::memcpy(pair_off, tsp.pair_off.data(), tsp.pair_off.size() * sizeof(uint64_t));
    if (seg_forget) std::memcpy(seg_forget, tsp.seg_forget.data(), tsp.seg_forget.size() * sizeof(uint32_t));
    return tsp.n_forget;
}
uint32_t qt_class_sample_tiled_pass(int state_bits, uint64_t bytes_per_job, uint64_t jobs_left, uint64_t cap)
{
    return sample::tiled_sample_pass_jobs(state_bits, bytes_per_job, jobs_left, cap ? cap : sample::kTiledSampleRecordBytes);
}
// the top rung's frames of a pick window (wu_frames.hpp) for an accepted scan = wave block, from the window's 64 pick blocks picks[64][4]: the plan's
// descriptors and logical masks (rows padded to the kernel's WV words, as the kernel stages them), thr16 from the plan's thr_logical as wu_run forms it.
// Writes frames[128 / iters][WV + 1] and returns WV; -1: refused, an unsupported width, or too small a buffer
int qt_wave_frames(const qecmc_params *p, const uint32_t *picks, uint32_t *frames, int cap)
{
    HostPlan hp;
    if (validate_params(p).code || plan_host(*p, hp).code || p->scan != QECMC_SCAN_WAVE) return -1;
    const LadderArgs &a = hp.args;
    const int L = a.L, W = a.W, WV = wu_words(W);
    const uint32_t steps = 128u / a.iters, thr16 = (uint32_t)((a.thr_logical + 65535u) >> 16);
    if (WV > 16 || (int)(steps * (uint32_t)(WV + 1)) > cap) return -1;
    std::vector<uint32_t> lml((size_t)4 * (L + 1) * WV, 0u);
    for (int row = 0; row < 4 * (L + 1); ++row)
        for (int w = 0; w < W; ++w) lml[(size_t)row * WV + w] = hp.lmask[(size_t)row * W + w];
#define QT_FRAMES(CODE, WVC) if (a.code == CODE && WV == WVC) wu_build_frames<CODE, WVC>(picks, a.iters, thr16, a.n_gen, L, hp.wu_desc.data(), lml.data(), frames);
#define QT_FRAMES_W(CODE) QT_FRAMES(CODE, 4) QT_FRAMES(CODE, 8) QT_FRAMES(CODE, 12) QT_FRAMES(CODE, 16)
    QT_FRAMES_W(kCodeToric) QT_FRAMES_W(kCodeXzzx) QT_FRAMES_W(kCodeRotated) QT_FRAMES_W(kCodePlanar)
#undef QT_FRAMES_W
#undef QT_FRAMES
    return WV;
}
// the swap sweep's bound of rung pair `pair` (wu_bounds.hpp) for an accepted scan = wave block under the depolarizing rule, on n words xs: the pair's row of
// swapT as the kernels stage it (ladder_wu_body.inc), the plan's swap_thr behind it, the plan's swap_inv_log2.  Returns nq; -1: refused or no such pair
int qt_wave_swap_bound(const qecmc_params *p, int pair, const uint32_t *xs, uint64_t n, uint32_t *out)
{
    HostPlan hp;
    if (validate_params(p).code || plan_host(*p, hp).code || p->scan != QECMC_SCAN_WAVE || p->noise != QECMC_NOISE_DEPOLARIZING) return -1;
    const LadderArgs &a = hp.args;
    if (pair < 0 || pair + 1 >= a.Nc || !a.swap_fast_ok) return -1;
    const int nq = a.nq;
    const uint64_t *thr = hp.swap_thr.data() + (size_t)pair * (nq + 1);
    uint32_t row[kSwapFast];
    for (int d = 0; d < kSwapFast; ++d) row[d] = (d >= 1 && d <= nq) ? (uint32_t)thr[d] : 0u;
    for (uint64_t k = 0; k < n; ++k)
        out[k] = wu_swap_bound(xs[k], a.swap_inv_log2[pair], nq, [&](int d) { return row[d]; }, [&](int d) { return (uint32_t)thr[d]; });
    return nq;
}
// ... and the pair's row of the plan's thresholds, swap_thr[pair][0 .. nq]: returns nq + 1; -1: refused, no such pair, or too small a buffer
int qt_wave_swap_row(const qecmc_params *p, int pair, uint64_t *out, int cap)
{
    HostPlan hp;
    if (validate_params(p).code || plan_host(*p, hp).code || p->scan != QECMC_SCAN_WAVE) return -1;
    const LadderArgs &a = hp.args;
    if (pair < 0 || pair + 1 >= a.Nc || cap < a.nq + 1) return -1;
    for (int d = 0; d <= a.nq; ++d) out[d] = hp.swap_thr[(size_t)pair * (a.nq + 1) + d];
    return a.nq + 1;
}
}
