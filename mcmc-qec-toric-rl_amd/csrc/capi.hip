// C-ABI of libqecmc (include/qecmc.h): argument checking, host-side threshold
// tables, device buffers and kernel launches.  No CPU compute fallback: every
// entry point that computes needs a HIP device.
#include "../../include/qecmc.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "plan_host.hpp"
#include "stencil_bytes.hpp"
#include "corrections.hpp"
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
#include "enumerate.hpp"
#include "syndrome_lift.hpp"
#include "tables.hpp"

using namespace qecmc;
using namespace qecmc::tables;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(QECMC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

int use_device(int dev)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(QECMC_ERR_NO_DEVICE, "no HIP device visible: libqecmc has no CPU fallback");
    if (dev < 0 || dev >= n) return fail(QECMC_ERR_NO_DEVICE, "device %d out of range (0..%d)", dev, n - 1);
    HIP_TRY(hipSetDevice(dev));
    return 0;
}

// Small device blocks are recycled: the drop-in entry points (one chain or one ladder per call, mcmc.py:81-103 driven from a Python loop)
// would otherwise spend most of a call in hipMalloc / hipFree -- hipFree also waits for the device.  Blocks up to kPoolBlock bytes are
// rounded up to a power of two and kept, per device, until kPoolBytes are cached; larger ones (the batched calls) go to the runtime as before.
// Nothing here is zero-filled, exactly like hipMalloc: every user writes its buffer before a kernel reads it.
class DevPool {
public:
    static constexpr size_t kPoolBlock = size_t(1) << 20, kPoolBytes = size_t(32) << 20;
    static DevPool &get() { static DevPool *pool = new DevPool; return *pool; }   // (never destroyed: the HIP runtime may be gone before static destructors run)
    hipError_t take(size_t bytes, void **p, size_t *cap, int *dev)
    {
        *cap = 0;
        if (bytes > kPoolBlock) return hipMalloc(p, bytes);
        size_t want = 256;
        while (want < bytes) want <<= 1;
        if (hipError_t e = hipGetDevice(dev)) return e;
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t i = 0; i < free_.size(); ++i)
                if (free_[i].cap == want && free_[i].dev == *dev) {
                    *p = free_[i].p; *cap = want;
                    cached_ -= want;
                    free_[i] = free_.back(); free_.pop_back();
                    return hipSuccess;
                }
        }
        *cap = want;
        return hipMalloc(p, want);
    }
    void give(void *p, size_t cap, int dev)
    {
        if (cap) {
            std::lock_guard<std::mutex> g(mu_);
            if (cached_ + cap <= kPoolBytes) { free_.push_back({p, cap, dev}); cached_ += cap; return; }
        }
        (void)hipFree(p);
    }
private:
    struct Blk { void *p; size_t cap; int dev; };
    std::mutex mu_;
    std::vector<Blk> free_;
    size_t cached_ = 0;
};

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;          // pooled block size (0: straight from hipMalloc)
    int dev = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) DevPool::get().give(p, cap, dev); }
    hipError_t alloc(size_t bytes) { return DevPool::get().take(bytes ? bytes : 1, &p, &cap, &dev); }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// kernel time of a launch on the null stream between start() and stop(); the events go on every path
struct EventTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventTimer() = default;
    EventTimer(const EventTimer &) = delete;
    EventTimer &operator=(const EventTimer &) = delete;
    ~EventTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    hipError_t start()
    {
        if (hipError_t e = hipEventCreate(&e0)) return e;
        if (hipError_t e = hipEventCreate(&e1)) return e;
        return hipEventRecord(e0, 0);
    }
    hipError_t stop(float *ms)
    {
        if (hipError_t e = hipEventRecord(e1, 0)) return e;
        if (hipError_t e = hipEventSynchronize(e1)) return e;
        return hipEventElapsedTime(ms, e0, e1);
    }
};

// a refusal of the host-only checks (plan_host.hpp), handed to qecmc_last_error()
int report(const Refusal &r) { return r.code ? fail(r.code, "%s", r.msg.c_str()) : 0; }

}  // namespace

struct qecmc_plan {
    qecmc_params prm;
    LadderArgs args;
    DevBuf swap_thr, lmask, acc_top, gen, bias, lnb, xyz_lut, gen_type, queue, phases, wu_desc, col_thr;
    uint32_t queue_grid = 0;                                   // persistent grid of the work-queue kernels (0: not a queue plan)
    size_t lds_bytes;
    uint32_t *d_swap_acc = nullptr, *d_nerr_sum = nullptr;   // qecmc_plan_set_stats (caller-owned)
    // qecmc_plan_set_shortest (caller-owned): the outputs, the ladders' sets and what a ladder may offer
    double *d_short_neff = nullptr;
    uint32_t *d_short_n = nullptr, *d_short_uniq = nullptr;
    uint8_t *d_short_over = nullptr;
    void *d_short_set = nullptr;
    uint64_t short_set_bytes = 0, short_cap = 0;
    // (plan_host.hpp: whether a launch runs on the persistent grid, and THE workspace formula of the criterion runs)
    bool takes_queue(bool wants_states_or_stats) const { return launch_takes_queue(queue_grid, prm.steps, wants_states_or_stats); }
    uint64_t workspace(uint64_t N, bool queue) const { return workspace_need(prm, queue_grid, N, queue); }
};

// the lift table of one (code, L) on the device (syndrome_lift.hpp): rows [cells][W + 1], the generator table, the launch's dimensions
struct qecmc_lift {
    LiftArgs args = {};
    DevBuf rows, gen;
};

// the correction tables of one (code, L) on the device (corrections.hpp): the logical masks [4][L+1][W], the class-move table, the generator table
struct qecmc_corrector {
    CorrectArgs args = {};
    DevBuf masks, need, gen;
};

namespace {

// the plan of a parameter block validate_params() accepts: plan_host() decides everything, this uploads its tables
int build_plan(const qecmc_params *p, qecmc_plan *pl)
{
    pl->prm = *p;
    HostPlan hp;
    if (int rc = report(plan_host(*p, hp))) return rc;
    LadderArgs &a = pl->args = hp.args;
    pl->lds_bytes = hp.lds_bytes;
    // (an empty table of the optional ones is one the plan does not have: its pointer stays null, which the launch path and the kernels test)
    auto upload = [](DevBuf &d, const auto &v, auto &dst, bool optional) -> int {
        if (optional && v.empty()) return 0;
        const size_t bytes = v.size() * sizeof v[0];
        HIP_TRY(d.alloc(bytes));
        HIP_TRY(hipMemcpy(d.p, v.data(), bytes, hipMemcpyHostToDevice));
        dst = static_cast<std::remove_reference_t<decltype(dst)>>(d.p);
        return 0;
    };
    int rc = 0;
    if ((rc = upload(pl->phases, hp.phases, a.phase_tab, true)) || (rc = upload(pl->wu_desc, hp.wu_desc, a.wu_desc, true)) ||
        (rc = upload(pl->gen, hp.gen, a.gen, false)) || (rc = upload(pl->bias, hp.bias, a.bias_tbl, true)) ||
        (rc = upload(pl->col_thr, hp.col_thr, a.col_thr, true)) || (rc = upload(pl->xyz_lut, hp.xyz_lut, a.xyz_lut, true)) ||
        (rc = upload(pl->gen_type, hp.gen_type, a.gen_type, true)) || (rc = upload(pl->lnb, hp.lnb, a.alpha_lnb, true)) ||
        (rc = upload(pl->swap_thr, hp.swap_thr, a.swap_thr, false)) || (rc = upload(pl->lmask, hp.lmask, a.lmask, false)) ||
        (rc = upload(pl->acc_top, hp.acc_top, a.acc_tbl_top, false)))
        return rc;
    if (!same_shape(kernel_shape(a), hp.shape)) return fail(QECMC_ERR_HIP, "internal: the uploaded plan's kernel shape differs from the host plan's");
    if (hp.takes_queue) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, p->device));
        pl->queue_grid = queue_grid(hp, prop.multiProcessorCount, p->flags);
        if (hp.queue_family == kFamLadder) HIP_TRY(pl->queue.alloc(sizeof(uint32_t)));
    }
    return 0;
}

}  // namespace

extern "C" {

int qecmc_abi_version(void) { return QECMC_ABI_VERSION; }
const char *qecmc_last_error(void) { return g_err.c_str(); }
int qecmc_last_kernel(int64_t key_out[10])
{
    KernelKey k;
    if (!key_out) return fail(QECMC_ERR_INVALID, "qecmc_last_kernel: NULL key_out");
    if (!last_launched_kernel(k)) return fail(QECMC_ERR_INVALID, "qecmc_last_kernel: this thread has launched no ladder kernel");
    const int64_t v[10] = {k.family, k.maxt, k.minw, k.code, k.flags, k.wv, k.conv, k.it, k.alpha, k.rule};
    memcpy(key_out, v, sizeof v);
    return QECMC_OK;
}
int qecmc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------- primitives
#define PRIM_PROLOGUE()                                   \
    if (int rc = report(check_code_L(code, L))) return rc; \
    if (int rc = use_device(0)) return rc;                \
    const size_t nq = code_nq(code, L);                   \
    (void)nq;                                             \
    if (N == 0) return 0

int qecmc_apply_stabilizer(int code, int L, uint64_t N, const uint8_t *in, uint8_t *out, const int32_t *rows,
                           const int32_t *cols, const int32_t *ops, int32_t *dE)
{
    PRIM_PROLOGUE();
    if (!in || !out || !rows || !cols || !ops || !dE) return fail(QECMC_ERR_INVALID, "NULL buffer");
    for (uint64_t i = 0; i < N; ++i) {
        if (ops[i] != 1 && ops[i] != 3) return fail(QECMC_ERR_INVALID, "stabilizer %llu: operator %d is not 1 or 3", (unsigned long long)i, ops[i]);
        const int rmax = code == QECMC_TORIC ? L : code == QECMC_PLANAR ? (ops[i] == 1 ? L - 1 : L) : (ops[i] == 1 ? L - 1 : (L - 1) / 2);
        const int cmax = code == QECMC_TORIC ? L : code == QECMC_PLANAR ? (ops[i] == 1 ? L : L - 1) : (ops[i] == 1 ? L - 1 : 4);
        if (rows[i] < 0 || rows[i] >= rmax || cols[i] < 0 || cols[i] >= cmax) return fail(QECMC_ERR_INVALID, "stabilizer %llu: (row,col)=(%d,%d) outside [0,%d)x[0,%d)", (unsigned long long)i, rows[i], cols[i], rmax, cmax);
    }
    DevBuf din, dout, dr, dc, dop, dd;
    HIP_TRY(din.alloc(N * nq)); HIP_TRY(dout.alloc(N * nq));
    HIP_TRY(dr.alloc(N * 4)); HIP_TRY(dc.alloc(N * 4)); HIP_TRY(dop.alloc(N * 4)); HIP_TRY(dd.alloc(N * 4));
    HIP_TRY(hipMemcpy(din.p, in, N * nq, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dr.p, rows, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dc.p, cols, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dop.p, ops, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(launch_apply_stabilizer(code, L, N, din.as<uint8_t>(), dout.as<uint8_t>(), dr.as<int32_t>(), dc.as<int32_t>(), dop.as<int32_t>(), dd.as<int32_t>(), 0));
    HIP_TRY(hipMemcpy(out, dout.p, N * nq, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dE, dd.p, N * 4, hipMemcpyDeviceToHost));
    return 0;
}

int qecmc_apply_logical(int code, int L, uint64_t N, const uint8_t *in, uint8_t *out, const int32_t *ops,
                        const int32_t *layers, const int32_t *xpos, const int32_t *zpos, int32_t *dE)
{
    PRIM_PROLOGUE();
    if (!in || !out || !ops || !layers || !xpos || !zpos || !dE) return fail(QECMC_ERR_INVALID, "NULL buffer");
    for (uint64_t i = 0; i < N; ++i) {
        if (ops[i] < 0 || ops[i] > 3) return fail(QECMC_ERR_INVALID, "logical %llu: operator %d outside [0,3]", (unsigned long long)i, ops[i]);
        if (layers[i] != 0 && layers[i] != 1) return fail(QECMC_ERR_INVALID, "logical %llu: layer %d is not 0 or 1", (unsigned long long)i, layers[i]);
        if (xpos[i] < 0 || xpos[i] >= L || zpos[i] < 0 || zpos[i] >= L) return fail(QECMC_ERR_INVALID, "logical %llu: position outside [0,%d)", (unsigned long long)i, L);
    }
    DevBuf din, dout, d0, d1, d2, d3, dd;
    HIP_TRY(din.alloc(N * nq)); HIP_TRY(dout.alloc(N * nq));
    HIP_TRY(d0.alloc(N * 4)); HIP_TRY(d1.alloc(N * 4)); HIP_TRY(d2.alloc(N * 4)); HIP_TRY(d3.alloc(N * 4)); HIP_TRY(dd.alloc(N * 4));
    HIP_TRY(hipMemcpy(din.p, in, N * nq, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d0.p, ops, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d1.p, layers, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d2.p, xpos, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d3.p, zpos, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(launch_apply_logical(code, L, N, din.as<uint8_t>(), dout.as<uint8_t>(), d0.as<int32_t>(), d1.as<int32_t>(), d2.as<int32_t>(), d3.as<int32_t>(), dd.as<int32_t>(), 0));
    HIP_TRY(hipMemcpy(out, dout.p, N * nq, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dE, dd.p, N * 4, hipMemcpyDeviceToHost));
    return 0;
}

int qecmc_count_errors(int code, int L, uint64_t N, const uint8_t *in, int64_t *n)
{
    PRIM_PROLOGUE();
    if (!in || !n) return fail(QECMC_ERR_INVALID, "NULL buffer");
    DevBuf din, dn;
    HIP_TRY(din.alloc(N * nq)); HIP_TRY(dn.alloc(N * 8));
    HIP_TRY(hipMemcpy(din.p, in, N * nq, hipMemcpyHostToDevice));
    HIP_TRY(launch_count_errors((int)nq, N, din.as<uint8_t>(), dn.as<int64_t>(), 0));
    HIP_TRY(hipMemcpy(n, dn.p, N * 8, hipMemcpyDeviceToHost));
    return 0;
}

int qecmc_eq_class(int code, int L, uint64_t N, const uint8_t *in, int32_t *cls)
{
    PRIM_PROLOGUE();
    if (!in || !cls) return fail(QECMC_ERR_INVALID, "NULL buffer");
    DevBuf din, dc;
    HIP_TRY(din.alloc(N * nq)); HIP_TRY(dc.alloc(N * 4));
    HIP_TRY(hipMemcpy(din.p, in, N * nq, hipMemcpyHostToDevice));
    HIP_TRY(launch_eq_class(code, L, N, din.as<uint8_t>(), dc.as<int32_t>(), 0));
    HIP_TRY(hipMemcpy(cls, dc.p, N * 4, hipMemcpyDeviceToHost));
    return 0;
}

int qecmc_to_class(int code, int L, uint64_t N, const uint8_t *in, uint8_t *out, const int32_t *eq)
{
    PRIM_PROLOGUE();
    if (!in || !out || !eq) return fail(QECMC_ERR_INVALID, "NULL buffer");
    if (code != QECMC_TORIC) return fail(QECMC_ERR_UNSUPPORTED, "to_class exists for the toric code only (toric_model.py:354)");
    for (uint64_t i = 0; i < N; ++i)
        if (eq[i] < 0 || eq[i] > 15) return fail(QECMC_ERR_INVALID, "to_class %llu: class %d outside [0,16)", (unsigned long long)i, eq[i]);
    DevBuf din, dout, de;
    HIP_TRY(din.alloc(N * nq)); HIP_TRY(dout.alloc(N * nq)); HIP_TRY(de.alloc(N * 4));
    HIP_TRY(hipMemcpy(din.p, in, N * nq, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(de.p, eq, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(launch_to_class(L, N, din.as<uint8_t>(), dout.as<uint8_t>(), de.as<int32_t>(), 0));
    HIP_TRY(hipMemcpy(out, dout.p, N * nq, hipMemcpyDeviceToHost));
    return 0;
}

int qecmc_syndrome(int code, int L, uint64_t N, const uint8_t *in, uint8_t *defects_out)
{
    PRIM_PROLOGUE();
    if (!in || !defects_out) return fail(QECMC_ERR_INVALID, "NULL buffer");
    const size_t nd = code == QECMC_TORIC ? nq : code == QECMC_PLANAR ? (size_t)2 * L * (L - 1) : (size_t)(L + 1) * (L + 1);
    DevBuf din, dout;
    HIP_TRY(din.alloc(N * nq)); HIP_TRY(dout.alloc(N * nd));
    HIP_TRY(hipMemcpy(din.p, in, N * nq, hipMemcpyHostToDevice));
    HIP_TRY(launch_syndrome(code, L, N, din.as<uint8_t>(), dout.as<uint8_t>(), 0));
    HIP_TRY(hipMemcpy(defects_out, dout.p, N * nd, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------- syndrome generation
static int generate_args(int code, int L, uint64_t N, double p_x, double p_y, double p_z, int hide_class, uint64_t seed,
                         uint32_t first_syndrome, GenArgs &a)
{
    if (int rc = report(check_code_L(code, L))) return rc;
    if (!(p_x >= 0.0) || !(p_y >= 0.0) || !(p_z >= 0.0) || !(p_x + p_y + p_z <= 1.0))
        return fail(QECMC_ERR_INVALID, "(p_x, p_y, p_z) = (%g, %g, %g) must be non-negative with a sum <= 1", p_x, p_y, p_z);
    if (code == QECMC_TORIC && !(p_x == p_y && p_y == p_z))
        return fail(QECMC_ERR_INVALID, "the toric model's generate_random_error(p) draws the Pauli uniformly (toric_model.py:15-23): pass p_x = p_y = p_z = p / 3");
    if (N + first_syndrome > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "global syndrome index exceeds 32 bits");
    std::memset(&a, 0, sizeof a);
    a.N = N; a.code = code; a.L = L; a.nq = (int)code_nq(code, L); a.hide = hide_class != 0;
    a.first_syndrome = first_syndrome; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    if (code == QECMC_TORIC) a.thr_z = thr64((p_x + p_y) + p_z);
    else { a.thr_z = thr64(p_z); a.thr_zx = thr64(p_z + p_x); a.thr_zxy = thr64((p_z + p_x) + p_y); }
    return 0;
}

int qecmc_generate_syndromes_dev(int code, int L, uint64_t N, double p_x, double p_y, double p_z, int hide_class, uint64_t seed,
                                 uint32_t first_syndrome, void *d_init_out, void *d_raw_out, void *d_eq_true_out, void *hip_stream)
{
    GenArgs a;
    if (int rc = generate_args(code, L, N, p_x, p_y, p_z, hide_class, seed, first_syndrome, a)) return rc;
    if (N == 0) return 0;
    if (!d_init_out) return fail(QECMC_ERR_INVALID, "NULL device buffer");
    a.out = static_cast<uint8_t *>(d_init_out); a.raw = static_cast<uint8_t *>(d_raw_out); a.eq_true = static_cast<int32_t *>(d_eq_true_out);
    HIP_TRY(launch_generate(a, static_cast<hipStream_t>(hip_stream)));
    return 0;
}

int qecmc_generate_syndromes(int code, int L, uint64_t N, double p_x, double p_y, double p_z, int hide_class, uint64_t seed,
                             uint32_t first_syndrome, uint8_t *init_out, uint8_t *raw_out, int32_t *eq_true_out)
{
    GenArgs a;
    if (int rc = generate_args(code, L, N, p_x, p_y, p_z, hide_class, seed, first_syndrome, a)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if (!init_out) return fail(QECMC_ERR_INVALID, "NULL buffer");
    const size_t nq = (size_t)a.nq;
    DevBuf dout, draw, deq;
    HIP_TRY(dout.alloc(N * nq));
    if (raw_out) HIP_TRY(draw.alloc(N * nq));
    if (eq_true_out) HIP_TRY(deq.alloc(N * 4));
    a.out = dout.as<uint8_t>(); a.raw = raw_out ? draw.as<uint8_t>() : nullptr; a.eq_true = eq_true_out ? deq.as<int32_t>() : nullptr;
    HIP_TRY(launch_generate(a, 0));
    HIP_TRY(hipMemcpy(init_out, dout.p, N * nq, hipMemcpyDeviceToHost));
    if (raw_out) HIP_TRY(hipMemcpy(raw_out, draw.p, N * nq, hipMemcpyDeviceToHost));
    if (eq_true_out) HIP_TRY(hipMemcpy(eq_true_out, deq.p, N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------- start chains from bare syndromes (syndrome_lift.hpp)
static int lift_upload(int code, int L, qecmc_lift *lf)
{
    const lift::Table t = lift::build_table(code, L);
    if (t.rows.empty()) return fail(QECMC_ERR_UNSUPPORTED, "internal: no lift table for code %d, L=%d", code, L);
    lf->args.N = 0; lf->args.n_cells = t.n_cells; lf->args.W = t.W; lf->args.nq = t.nq; lf->args.n_gen = t.n_gen; lf->args.descend = 0;
    HIP_TRY(lf->rows.alloc(t.rows.size() * sizeof(uint32_t)));
    HIP_TRY(lf->gen.alloc(t.gen.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(lf->rows.p, t.rows.data(), t.rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lf->gen.p, t.gen.data(), t.gen.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
}

static int lift_launch(const qecmc_lift *lf, const void *d_defects, uint64_t N, int descend, void *d_chains, void *d_status, void *d_weight, hipStream_t s)
{
    LiftArgs a = lf->args;
    a.N = N; a.descend = descend != 0;
    HIP_TRY(launch_syndrome_lift(a, lf->rows.as<uint32_t>(), lf->gen.as<uint32_t>(), static_cast<const uint8_t *>(d_defects), static_cast<uint8_t *>(d_chains),
                                 static_cast<uint8_t *>(d_status), static_cast<int32_t *>(d_weight), s));
    return 0;
}

int qecmc_lift_create(int code, int L, qecmc_lift **out)
{
    if (!out) return fail(QECMC_ERR_INVALID, "qecmc_lift_create: NULL out");
    *out = nullptr;
    if (int rc = report(check_code_L(code, L))) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(QECMC_ERR_NO_DEVICE, "no HIP device visible: libqecmc has no CPU fallback");
    std::unique_ptr<qecmc_lift> lf(new (std::nothrow) qecmc_lift);
    if (!lf) return fail(QECMC_ERR_INVALID, "out of host memory");
    if (int rc = lift_upload(code, L, lf.get())) return rc;
    *out = lf.release();
    return 0;
}

int qecmc_lift_destroy(qecmc_lift *lift)
{
    delete lift;
    return 0;
}

int qecmc_chains_from_syndromes_dev(qecmc_lift *lift, const void *d_defects, uint64_t N, int descend, void *d_chains_out, void *d_status_out,
                                    void *d_weight_out, void *hip_stream)
{
    if (!lift) return fail(QECMC_ERR_INVALID, "qecmc_chains_from_syndromes_dev: NULL lift");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    if (N == 0) return 0;
    if (!d_defects || !d_chains_out) return fail(QECMC_ERR_INVALID, "NULL device buffer");
    return lift_launch(lift, d_defects, N, descend, d_chains_out, d_status_out, d_weight_out, static_cast<hipStream_t>(hip_stream));
}

int qecmc_chains_from_syndromes(int code, int L, uint64_t N, const uint8_t *defects, int descend, uint8_t *chains_out, uint8_t *status_out,
                                int32_t *weight_out)
{
    if (!defects || !chains_out) return fail(QECMC_ERR_INVALID, "qecmc_chains_from_syndromes: NULL buffer");
    if (int rc = report(check_code_L(code, L))) return rc;
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    qecmc_lift lf;
    if (int rc = lift_upload(code, L, &lf)) return rc;
    const size_t nq = (size_t)lf.args.nq, nd = (size_t)lf.args.n_cells;
    DevBuf din, dout, dst, dw;
    HIP_TRY(din.alloc(N * nd)); HIP_TRY(dout.alloc(N * nq)); HIP_TRY(dst.alloc(N)); HIP_TRY(dw.alloc(N * 4));
    HIP_TRY(hipMemcpy(din.p, defects, N * nd, hipMemcpyHostToDevice));
    if (int rc = lift_launch(&lf, din.p, N, descend, dout.p, dst.p, dw.p, 0)) return rc;
    HIP_TRY(hipMemcpy(chains_out, dout.p, N * nq, hipMemcpyDeviceToHost));
    if (status_out) HIP_TRY(hipMemcpy(status_out, dst.p, N, hipMemcpyDeviceToHost));
    if (weight_out) HIP_TRY(hipMemcpy(weight_out, dw.p, N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------- corrections from decoded syndromes (corrections.hpp)
// the host half: INVALID for a (code, L) the library does not know, UNSUPPORTED where the logical operators do not reach every class
static int corrector_table(int code, int L, correct::Table &t)
{
    if (int rc = report(check_code_L(code, L))) return rc;
    t = correct::build_table(code, L);
    if (t.need.empty())
        return fail(QECMC_ERR_UNSUPPORTED, "no class move for code %d at L=%d: its logical operators do not reach every equivalence class (the toric code's "
                                           "parity class does not see a logical line of even length)", code, L);
    return 0;
}

static int corrector_upload(const correct::Table &t, qecmc_corrector *c)
{
    CorrectArgs &a = c->args;
    a.N = 0; a.code = t.code; a.L = t.L; a.W = t.W; a.nq = t.nq; a.n_gen = t.n_gen; a.ncls = t.ncls; a.kinds = t.kinds; a.K = 1; a.place = 0; a.descend = 0;
    HIP_TRY(c->masks.alloc(t.masks.size() * sizeof(uint32_t)));
    HIP_TRY(c->need.alloc(t.need.size() * sizeof(uint32_t)));
    HIP_TRY(c->gen.alloc(t.gen.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(c->masks.p, t.masks.data(), t.masks.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->need.p, t.need.data(), t.need.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->gen.p, t.gen.data(), t.gen.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
}

static int corrector_launch(const qecmc_corrector *c, const void *d_candidates, const void *d_target, uint64_t N, uint32_t K, int place, int descend,
                            void *d_out, void *d_weight, void *d_source, void *d_moved, void *d_status, hipStream_t s)
{
    CorrectArgs a = c->args;
    a.N = N; a.K = (int)K; a.place = place != 0; a.descend = descend != 0;
    HIP_TRY(launch_corrections(a, c->masks.as<uint32_t>(), c->need.as<uint32_t>(), c->gen.as<uint32_t>(), static_cast<const uint8_t *>(d_candidates),
                               static_cast<const int32_t *>(d_target), static_cast<uint8_t *>(d_out), static_cast<int32_t *>(d_weight),
                               static_cast<int32_t *>(d_source), static_cast<uint8_t *>(d_moved), static_cast<uint8_t *>(d_status), s));
    return 0;
}

// (K candidates of nq <= 8192 bytes per syndrome: K * nq stays below 2^31)
static int check_corrections_size(uint64_t N, uint32_t K)
{
    if (K == 0) return fail(QECMC_ERR_INVALID, "K=0: a correction needs at least one candidate chain");
    if (K > 0xFFFFu) return fail(QECMC_ERR_INVALID, "K=%u candidates per syndrome exceed 65535", K);
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    return 0;
}

int qecmc_corrector_create(int code, int L, qecmc_corrector **out)
{
    if (!out) return fail(QECMC_ERR_INVALID, "qecmc_corrector_create: NULL out");
    *out = nullptr;
    correct::Table t;
    if (int rc = corrector_table(code, L, t)) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(QECMC_ERR_NO_DEVICE, "no HIP device visible: libqecmc has no CPU fallback");
    std::unique_ptr<qecmc_corrector> c(new (std::nothrow) qecmc_corrector);
    if (!c) return fail(QECMC_ERR_INVALID, "out of host memory");
    if (int rc = corrector_upload(t, c.get())) return rc;
    *out = c.release();
    return 0;
}

int qecmc_corrector_destroy(qecmc_corrector *c)
{
    delete c;
    return 0;
}

int qecmc_corrections_dev(qecmc_corrector *c, const void *d_candidates, const void *d_target, uint64_t N, uint32_t K, int place, int descend,
                          void *d_corrections_out, void *d_weight_out, void *d_source_out, void *d_moved_out, void *d_status_out, void *hip_stream)
{
    if (!c) return fail(QECMC_ERR_INVALID, "qecmc_corrections_dev: NULL corrector");
    if (int rc = check_corrections_size(N, K)) return rc;
    if (N == 0) return 0;
    if (!d_candidates || !d_target || !d_corrections_out) return fail(QECMC_ERR_INVALID, "NULL device buffer");
    return corrector_launch(c, d_candidates, d_target, N, K, place, descend, d_corrections_out, d_weight_out, d_source_out, d_moved_out, d_status_out,
                            static_cast<hipStream_t>(hip_stream));
}

int qecmc_corrections(int code, int L, uint64_t N, uint32_t K, const uint8_t *candidates, const int32_t *target, int place, int descend,
                      uint8_t *corrections_out, int32_t *weight_out, int32_t *source_out, uint8_t *moved_out, uint8_t *status_out)
{
    if (!candidates || !target || !corrections_out) return fail(QECMC_ERR_INVALID, "qecmc_corrections: NULL buffer");
    if (int rc = check_corrections_size(N, K)) return rc;
    correct::Table t;
    if (int rc = corrector_table(code, L, t)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    qecmc_corrector c;
    if (int rc = corrector_upload(t, &c)) return rc;
    const size_t nq = (size_t)t.nq;
    DevBuf din, dt, dout, dw, ds, dm, dst;
    HIP_TRY(din.alloc(N * K * nq)); HIP_TRY(dt.alloc(N * 4)); HIP_TRY(dout.alloc(N * nq));
    HIP_TRY(dw.alloc(N * 4)); HIP_TRY(ds.alloc(N * 4)); HIP_TRY(dm.alloc(N)); HIP_TRY(dst.alloc(N));
    HIP_TRY(hipMemcpy(din.p, candidates, N * K * nq, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dt.p, target, N * 4, hipMemcpyHostToDevice));
    if (int rc = corrector_launch(&c, din.p, dt.p, N, K, place, descend, dout.p, dw.p, ds.p, dm.p, dst.p, 0)) return rc;
    HIP_TRY(hipMemcpy(corrections_out, dout.p, N * nq, hipMemcpyDeviceToHost));
    if (weight_out) HIP_TRY(hipMemcpy(weight_out, dw.p, N * 4, hipMemcpyDeviceToHost));
    if (source_out) HIP_TRY(hipMemcpy(source_out, ds.p, N * 4, hipMemcpyDeviceToHost));
    if (moved_out) HIP_TRY(hipMemcpy(moved_out, dm.p, N, hipMemcpyDeviceToHost));
    if (status_out) HIP_TRY(hipMemcpy(status_out, dst.p, N, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------- the exact class law by coset enumeration (enumerate.hpp)
int qecmc_coset_enumerate_info(int code, int L, int32_t *rank, int32_t *ncls, int32_t *nq, int32_t *default_chunk_bits)
{
    const enumr::Table t = enumr::build_table(code, L);
    if (int rc = report(t.refusal)) return rc;
    int bits = 0;
    uint64_t count = 0;
    if (int rc = report(enumr::resolve_range(t, bits, 0, count))) return rc;
    if (rank) *rank = t.rank;
    if (ncls) *ncls = t.ncls;
    if (nq) *nq = t.nq;
    if (default_chunk_bits) *default_chunk_bits = bits;
    return 0;
}

int qecmc_coset_enumerate(int code, int L, uint64_t N, const uint8_t *chains, int chunk_bits, uint64_t chunk_first, uint64_t chunk_count,
                          uint64_t *hist_out, int32_t *class_out)
{
    if (!chains || !hist_out) return fail(QECMC_ERR_INVALID, "qecmc_coset_enumerate: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    const enumr::Table t = enumr::build_table(code, L);
    if (int rc = report(t.refusal)) return rc;
    if (int rc = report(enumr::resolve_range(t, chunk_bits, chunk_first, chunk_count))) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    const enumr::Shape shape = enumr::launch_shape(t.ncls, chunk_bits, N);
    const size_t per = (size_t)t.carve.copy_words;                              // counters of one syndrome
    std::vector<uint32_t> gen((size_t)2 * t.rank), reps((size_t)shape.group * t.ncls * 2);
    for (int b = 0; b < t.rank; ++b) { gen[(size_t)2 * b] = t.gx[(size_t)b]; gen[(size_t)2 * b + 1] = t.gz[(size_t)b]; }
    DevBuf dgen, dreps, dhist;
    HIP_TRY(dgen.alloc(gen.size() * sizeof(uint32_t)));
    HIP_TRY(dreps.alloc(reps.size() * sizeof(uint32_t)));
    HIP_TRY(dhist.alloc((size_t)shape.group * per * sizeof(uint64_t)));
    HIP_TRY(hipMemcpy(dgen.p, gen.data(), gen.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    EnumArgs a = {};
    a.nq1 = (uint32_t)t.nq + 1u; a.bins = t.carve.bins; a.copies = t.carve.copies; a.ncls = t.ncls;
    a.chunk_bits = chunk_bits; a.slice_bits = shape.slice_bits; a.blocks = shape.blocks;
    // the host loops over groups of syndromes and over chunks: no launch, and no device block, grows with the batch
    for (uint64_t first = 0; first < N; first += shape.group) {
        const uint64_t here = N - first < shape.group ? N - first : shape.group;
        for (uint64_t s = 0; s < here; ++s) {
            const int cls = enumr::class_representatives(t, chains + (first + s) * (uint64_t)t.nq, reps.data() + s * (uint64_t)t.ncls * 2);
            if (class_out) class_out[first + s] = cls;
        }
        HIP_TRY(hipMemcpy(dreps.p, reps.data(), (size_t)here * t.ncls * 2 * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(dhist.p, 0, (size_t)here * per * sizeof(uint64_t), 0));   // (a block from the pool comes back dirty)
        a.S = (uint32_t)here;
        for (uint64_t k = chunk_first; k < chunk_first + chunk_count; ++k) {
            enumr::product_planes(t, chunk_bits, k, a.cx, a.cz);
            HIP_TRY(launch_enumerate(a, dgen.as<uint32_t>(), dreps.as<uint32_t>(), dhist.as<unsigned long long>(), 0));
        }
        HIP_TRY(hipMemcpy(hist_out + first * per, dhist.p, (size_t)here * per * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

// ---------------------------------------------------------------- the exact class law by a frontier sweep (class_sweep.hpp)
int qecmc_class_sweep_info(int code, int L, int32_t *width, int32_t *ncls, int32_t *nq, int32_t *n_ops)
{
    const sweep::Plan p = sweep::build_plan(code, L);
    if (int rc = report(p.refusal)) return rc;
    if (width) *width = p.width;
    if (ncls) *ncls = p.ncls;
    if (nq) *nq = p.nq;
    if (n_ops) *n_ops = p.n_ops;
    return 0;
}

extern "C++" {                                                                  // (templates)
namespace {
// What the ten entry points of the class sweeps share: the op words and the held words of the plan and the representatives of one launch group on
// the device, and the host loop over groups of syndromes -- no launch, and no device block, grows with the batch.
struct SweepBatch {
    const sweep::Plan &p;
    const uint32_t group;
    const size_t rep_words;                                                     // words of one syndrome's representatives
    std::vector<uint32_t> reps;
    DevBuf dops, dheld, dreps;
    SweepBatch(const sweep::Plan &plan, uint32_t syndromes) : p(plan), group(syndromes), rep_words((size_t)plan.ncls * plan.W), reps((size_t)syndromes * rep_words) {}
    // the three blocks, and the uploads that do not change from group to group; held: nullptr where the route holds nothing
    int open(const std::vector<uint32_t> &ops, const std::vector<uint32_t> *held)
    {
        HIP_TRY(dops.alloc(ops.size() * sizeof(uint32_t)));
        if (held) HIP_TRY(dheld.alloc(held->size() * sizeof(uint32_t)));
        HIP_TRY(dreps.alloc(reps.size() * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(dops.p, ops.data(), ops.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (held && !held->empty()) HIP_TRY(hipMemcpy(dheld.p, held->data(), held->size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        return 0;
    }
    // per group: class_representatives per syndrome, their upload, then body(first, here) -- the entry point's launches and copies back
    template <class Body> int run(uint64_t N, const uint8_t *chains, int32_t *class_out, Body body)
    {
        for (uint64_t first = 0; first < N; first += group) {
            const uint64_t here = N - first < group ? N - first : group;
            for (uint64_t s = 0; s < here; ++s) {
                const int cls = sweep::class_representatives(p, chains + (first + s) * (uint64_t)p.nq, reps.data() + s * rep_words);
                if (class_out) class_out[first + s] = cls;
            }
            HIP_TRY(hipMemcpy(dreps.p, reps.data(), (size_t)here * rep_words * sizeof(uint32_t), hipMemcpyHostToDevice));
            if (int rc = body(first, here)) return rc;
        }
        return 0;
    }
    // `per` elements per (syndrome, class) of a group's results, to their place in the caller's array; out may be NULL
    template <class T> int fetch(T *out, const DevBuf &d, uint64_t first, uint64_t here, size_t per = 1) const
    {
        const size_t row = (size_t)p.ncls * per;
        if (out) HIP_TRY(hipMemcpy(out + first * row, d.p, (size_t)here * row * sizeof(T), hipMemcpyDeviceToHost));
        return 0;
    }
    uint32_t *ops() const { return dops.as<uint32_t>(); }
    uint32_t *held() const { return dheld.as<uint32_t>(); }
    uint32_t *rep() const { return dreps.as<uint32_t>(); }
};

SweepCutArgs cut_args(const sweep::Plan &p, int n_held)
{
    SweepCutArgs a = {};
    a.ncls = p.ncls; a.W = p.W; a.width = p.width; a.n_ops = p.n_ops; a.n_held = n_held; a.scale = p.scale;
    return a;
}

MinplusArgs minplus_args(const sweep::Plan &p, int n_held)
{
    MinplusArgs a = {};
    a.ncls = p.ncls; a.W = p.W; a.width = p.width; a.n_ops = p.n_ops; a.n_held = n_held; a.shift = p.n_gen - p.rank;
    return a;
}
}  // namespace
}  // extern "C++"

int qecmc_class_sweep(int code, int L, uint64_t N, const uint8_t *chains, const double *w, double *z_out, int32_t *class_out)
{
    if (!chains || !w || !z_out) return fail(QECMC_ERR_INVALID, "qecmc_class_sweep: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    if (int rc = report(sweep::check_weights(w))) return rc;
    const sweep::Plan p = sweep::build_plan(code, L);
    if (int rc = report(p.refusal)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    SweepBatch b(p, sweep::launch_group(N));
    DevBuf dz;
    if (int rc = b.open(p.ops, nullptr)) return rc;
    HIP_TRY(dz.alloc((size_t)b.group * p.ncls * sizeof(double)));
    SweepArgs a = {};
    a.ncls = p.ncls; a.W = p.W; a.width = p.width; a.n_ops = p.n_ops; a.scale = p.scale;
    sweep::weights_xz(w, a.wxz);
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {     // every z of a group is written by its workgroup
        a.S = (uint32_t)here;
        HIP_TRY(launch_class_sweep(a, b.ops(), b.rep(), dz.as<double>(), 0));
        return b.fetch(z_out, dz, first, here);
    });
}

// ---------------------------------------------------------------- the frontier sweep past one LDS state vector (class_sweep_cut.hpp)
int qecmc_class_sweep_cut_info(int code, int L, int lds_width, int32_t *full_width, int32_t *width, int32_t *n_held, int32_t *ncls, int32_t *nq,
                               int32_t *n_ops)
{
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    if (int rc = report(cp.plan.refusal)) return rc;
    if (full_width) *full_width = cp.full_width;
    if (width) *width = cp.plan.width;
    if (n_held) *n_held = cp.n_held;
    if (ncls) *ncls = cp.plan.ncls;
    if (nq) *nq = cp.plan.nq;
    if (n_ops) *n_ops = cp.plan.n_ops;
    return 0;
}

int qecmc_class_sweep_cut(int code, int L, uint64_t N, const uint8_t *chains, const double *w, int lds_width, double *z_out, int32_t *class_out)
{
    if (!chains || !w || !z_out) return fail(QECMC_ERR_INVALID, "qecmc_class_sweep_cut: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    if (int rc = report(sweep::check_weights(w))) return rc;
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    const sweep::Plan &p = cp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if (class_sweep_cut_allow_lds(p.width) != hipSuccess)
        return fail(QECMC_ERR_UNSUPPORTED, "this device does not grant a workgroup the %u bytes of LDS a state vector of width %d takes", p.carve.bytes, p.width);
    SweepBatch b(p, sweep::cut_launch_group(N, p.ncls, cp.n_held));
    const size_t partials = (size_t)p.ncls << cp.n_held;                        // of one syndrome
    DevBuf dpart, dz;
    if (int rc = b.open(p.ops, &cp.held_words)) return rc;
    HIP_TRY(dpart.alloc((size_t)b.group * partials * sizeof(double)));          // kCutGridMax doubles at most; dirty: every partial is written before it is read
    HIP_TRY(dz.alloc((size_t)b.group * p.ncls * sizeof(double)));
    SweepCutArgs a = cut_args(p, cp.n_held);
    sweep::weights_xz(w, a.wxz);
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {
        a.S = (uint32_t)here;
        HIP_TRY(launch_class_sweep_cut(a, b.ops(), b.held(), b.rep(), dpart.as<double>(), dz.as<double>(), 0));
        return b.fetch(z_out, dz, first, here);
    });
}

// ---------------------------------------------------------------- shortest chains per class: the sweep in (min, +, count) (class_minplus.hpp)
int qecmc_class_minplus(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t cost[4], int lds_width, uint32_t *cost_out, uint64_t *count_out,
                        int32_t *class_out)
{
    if (!chains || !cost || !cost_out || !count_out) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus: N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    if (int rc = report(minplus::check_costs(cost))) return rc;
    const sweep::CutPlan cp = minplus::build_minplus_plan(code, L, lds_width);
    const sweep::Plan &p = cp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if (class_minplus_allow_lds(p.width) != hipSuccess)
        return fail(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus: this device does not grant a workgroup the %u bytes of LDS a state vector of width %d takes", p.carve.bytes,
                    p.width);
    SweepBatch b(p, sweep::cut_launch_group(N, p.ncls, cp.n_held));
    const size_t partials = (size_t)p.ncls << cp.n_held;                        // of one syndrome
    DevBuf dpart, dcost, dcount;
    if (int rc = b.open(p.ops, &cp.held_words)) return rc;
    HIP_TRY(dpart.alloc((size_t)b.group * partials * sizeof(uint64_t)));        // kCutGridMax entries at most; dirty: every partial is written before it is read
    HIP_TRY(dcost.alloc((size_t)b.group * p.ncls * sizeof(uint32_t)));
    HIP_TRY(dcount.alloc((size_t)b.group * p.ncls * sizeof(uint64_t)));
    MinplusArgs a = minplus_args(p, cp.n_held);
    minplus::costs_xz(cost, a.cxz);
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {
        a.S = (uint32_t)here;
        HIP_TRY(launch_class_minplus(a, b.ops(), b.held(), b.rep(), dpart.as<uint64_t>(), dcost.as<uint32_t>(), dcount.as<uint64_t>(), 0));
        if (int rc = b.fetch(cost_out, dcost, first, here)) return rc;
        return b.fetch(count_out, dcount, first, here);
    });
}

namespace {
// the device blocks of a traceback besides the sweep's: the forget words, the picks, the decision words and the chains of one launch group
struct TraceBlocks {
    DevBuf dforget, dpart, dpick, ddec, dchain, dcost, dcount;
    int open(const SweepBatch &b, const minplus::TracePlan &tp, uint64_t pair_bytes)
    {
        const sweep::Plan &p = b.p;
        const size_t pairs = (size_t)b.group * p.ncls;
        HIP_TRY(dforget.alloc(tp.forget_words.size() * sizeof(uint32_t)));
        HIP_TRY(dpart.alloc((pairs << tp.cut.n_held) * sizeof(uint64_t)));      // dirty: every partial is written before it is read
        HIP_TRY(dpick.alloc(pairs * sizeof(uint32_t)));
        HIP_TRY(ddec.alloc(pairs * (size_t)pair_bytes));                        // kTraceWorkspaceBytes at most; dirty: the walk reads what the trace wrote
        HIP_TRY(dchain.alloc(pairs * p.nq));
        HIP_TRY(dcost.alloc(pairs * sizeof(uint32_t)));
        HIP_TRY(dcount.alloc(pairs * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(dforget.p, tp.forget_words.data(), tp.forget_words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        return 0;
    }
    // the chains, and the costs and counts where the caller asked for them
    int fetch(const SweepBatch &b, uint64_t first, uint64_t here, uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out) const
    {
        if (int rc = b.fetch(chain_out, dchain, first, here, (size_t)b.p.nq)) return rc;
        if (int rc = b.fetch(cost_out, dcost, first, here)) return rc;
        return b.fetch(count_out, dcount, first, here);
    }
};
}  // namespace

// ---------------------------------------------------------------- a shortest chain per class: the (min, +) sweep traced back (class_minplus_trace.hpp)
int qecmc_class_minplus_chains(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t cost[4], int lds_width, uint8_t *chain_out, uint32_t *cost_out,
                               uint64_t *count_out, int32_t *class_out)
{
    if (!chains || !cost || !chain_out) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_chains: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_chains: N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    if (int rc = report(minplus::check_chain_costs(cost))) return rc;
    const minplus::TracePlan tp = minplus::build_trace_plan(code, L, lds_width);
    const sweep::CutPlan &cp = tp.cut;
    const sweep::Plan &p = cp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if (class_minplus_allow_lds(p.width) != hipSuccess || class_minplus_trace_allow_lds(p.width) != hipSuccess)
        return fail(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_chains: this device does not grant a workgroup the %u bytes of LDS a state vector of width %d takes",
                    p.carve.bytes, p.width);
    const uint64_t pair_bytes = minplus::trace_bytes_per_pair(tp);
    SweepBatch b(p, minplus::trace_launch_group(N, p.ncls, cp.n_held, pair_bytes));
    TraceBlocks d;
    if (int rc = b.open(p.ops, &cp.held_words)) return rc;
    if (int rc = d.open(b, tp, pair_bytes)) return rc;
    MinplusTraceArgs t = {};
    MinplusArgs &a = t.m;
    a = minplus_args(p, cp.n_held);
    minplus::costs_xz(cost, a.cxz);
    t.n_forget = tp.n_forget; t.words_per_forget = tp.words_per_forget; t.nq = p.nq;
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {
        a.S = (uint32_t)here;
        HIP_TRY(launch_class_minplus_sweep(a, b.ops(), b.held(), b.rep(), d.dpart.as<uint64_t>(), 0));
        HIP_TRY(launch_minplus_pick(a, d.dpart.as<uint64_t>(), d.dpick.as<uint32_t>(), 0));          // (before the reduce folds the partials in place)
        HIP_TRY(launch_class_minplus_reduce(a, d.dpart.as<uint64_t>(), d.dcost.as<uint32_t>(), d.dcount.as<uint64_t>(), 0));
        HIP_TRY(launch_minplus_trace(t, b.ops(), b.held(), b.rep(), d.dforget.as<uint32_t>(), d.dpick.as<uint32_t>(), d.ddec.as<uint64_t>(), d.dchain.as<uint8_t>(), 0));
        return d.fetch(b, first, here, chain_out, cost_out, count_out);
    });
}

// ---------------------------------------------------------------- the frontier sweep on a state vector tiled over HBM (class_sweep_tiled.hpp)
int qecmc_class_sweep_tiled_info(int code, int L, int hbm_width, int tile_width, int32_t *full_width, int32_t *width, int32_t *n_held, int32_t *ncls, int32_t *nq,
                                 int32_t *n_ops, int32_t *n_segments)
{
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (int rc = report(tp.plan.refusal)) return rc;
    if (full_width) *full_width = tp.full_width;
    if (width) *width = tp.plan.width;
    if (n_held) *n_held = tp.n_held;
    if (ncls) *ncls = tp.plan.ncls;
    if (nq) *nq = tp.plan.nq;
    if (n_ops) *n_ops = tp.plan.n_ops;
    if (n_segments) *n_segments = (int32_t)tp.segments.size();
    return 0;
}

namespace {
// The state vectors of the tiled sweep: one block per device, taken with one hipMalloc when a call first needs more than is there and kept -- it is
// kTiledWorkspaceBytes at most, and never cleared.  A call holds the lock from its first launch to its last copy.
struct TiledWorkspace {
    static constexpr int kDevices = 64;
    std::mutex mu;
    void *p[kDevices] = {};
    size_t bytes[kDevices] = {};
    static TiledWorkspace &get() { static TiledWorkspace *w = new TiledWorkspace; return *w; }      // (never destroyed, as DevPool)
    hipError_t take(size_t want, void **out)                                      // under mu
    {
        int dev = 0;
        if (hipError_t e = hipGetDevice(&dev)) return e;
        if (dev < 0 || dev >= kDevices || want > sweep::kTiledWorkspaceBytes) return hipErrorInvalidValue;
        if (bytes[dev] < want) {
            if (p[dev]) { (void)hipFree(p[dev]); p[dev] = nullptr; bytes[dev] = 0; }
            if (hipError_t e = hipMalloc(&p[dev], want)) return e;
            bytes[dev] = want;
        }
        *out = p[dev];
        return hipSuccess;
    }
};

extern "C++" {                                                                  // (a template)
// What the four tiled entry points share once the plan is accepted and the device chosen; T is the entry, a double or a packed (cost, count) word.
// open_rows(group): the caller's own blocks, after the sweep's; per_group(first, here): its per-group uploads; pass(unit_first, units, batch, work,
// partials): the launches of one pass of units; finish(batch, first, here, partials): the reduce of a group and its results' way back.  The host
// loops over groups of syndromes and, within a group, over passes of units: no launch, and no device block, grows with the batch.
template <class T, class OpenRows, class PerGroup, class Pass, class Finish>
int tiled_batch(const sweep::TiledPlan &tp, uint64_t N, const uint8_t *chains, int32_t *class_out, OpenRows open_rows, PerGroup per_group, Pass pass_launch, Finish finish)
{
    static_assert(sizeof(T) == sizeof(double), "one workspace, one cap and one pass size for every entry");
    const sweep::Plan &p = tp.plan;
    SweepBatch b(p, sweep::cut_launch_group(N, p.ncls, tp.n_held));
    const uint32_t pass = sweep::tiled_pass_units(tp.state_bits);
    const size_t partials = (size_t)p.ncls << tp.n_held;                        // of one syndrome
    const uint64_t group_units = (uint64_t)b.group * partials;
    DevBuf dpart;
    if (int rc = b.open(tp.dev_ops, &tp.held_words)) return rc;
    HIP_TRY(dpart.alloc((size_t)b.group * partials * sizeof(T)));               // kCutGridMax entries at most; dirty: every partial is written before it is read
    if (int rc = open_rows(b.group)) return rc;
    TiledWorkspace &ws = TiledWorkspace::get();                                 // one block, one cap of kTiledWorkspaceBytes and one lock for every entry point
    std::lock_guard<std::mutex> hold(ws.mu);
    void *work = nullptr;
    HIP_TRY(ws.take((size_t)(group_units < pass ? group_units : pass) * (sizeof(T) << tp.state_bits), &work));
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {
        const uint64_t units = here * partials;
        if (int rc = per_group(first, here)) return rc;
        for (uint64_t u = 0; u < units; u += pass)
            HIP_TRY(pass_launch((uint32_t)u, (uint32_t)(units - u < pass ? units - u : pass), b, static_cast<T *>(work), dpart.as<T>()));
        return finish(b, first, here, dpart.as<T>());
    });
}
}  // extern "C++"

// the end of a group of the two sum-product entry points: k_class_sweep_reduce, then Z to its place in the caller's array
struct TiledSum {
    SweepCutArgs ra;
    double *z_out;
    DevBuf dz;
    TiledSum(const sweep::TiledPlan &tp, double *z) : ra(cut_args(tp.plan, tp.n_held)), z_out(z) {}
    int open(uint32_t group) { HIP_TRY(dz.alloc((size_t)group * ra.ncls * sizeof(double))); return 0; }
    int operator()(const SweepBatch &b, uint64_t first, uint64_t here, double *P)
    {
        ra.S = (uint32_t)here;
        HIP_TRY(launch_class_sweep_reduce(ra, P, dz.as<double>(), 0));
        return b.fetch(z_out, dz, first, here);
    }
};

// ... and of the two (min, +) ones: k_class_minplus_reduce, then the costs and the counts
struct TiledFold {
    MinplusArgs ra;
    uint32_t *cost_out;
    uint64_t *count_out;
    DevBuf dcost, dcount;
    TiledFold(const sweep::TiledPlan &tp, uint32_t *cost, uint64_t *count) : ra(minplus_args(tp.plan, tp.n_held)), cost_out(cost), count_out(count) {}
    int open(uint32_t group)
    {
        HIP_TRY(dcost.alloc((size_t)group * ra.ncls * sizeof(uint32_t)));
        HIP_TRY(dcount.alloc((size_t)group * ra.ncls * sizeof(uint64_t)));
        return 0;
    }
    int operator()(const SweepBatch &b, uint64_t first, uint64_t here, uint64_t *P)
    {
        ra.S = (uint32_t)here;
        HIP_TRY(launch_class_minplus_reduce(ra, P, dcost.as<uint32_t>(), dcount.as<uint64_t>(), 0));
        if (int rc = b.fetch(cost_out, dcost, first, here)) return rc;
        return b.fetch(count_out, dcount, first, here);
    }
};
}  // namespace

int qecmc_class_sweep_tiled(int code, int L, uint64_t N, const uint8_t *chains, const double *w, int hbm_width, int tile_width, double *z_out, int32_t *class_out)
{
    if (!chains || !w || !z_out) return fail(QECMC_ERR_INVALID, "qecmc_class_sweep_tiled: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    if (int rc = report(sweep::check_weights(w))) return rc;
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    if (int rc = report(tp.plan.refusal)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    double wxz[4];
    sweep::weights_xz(w, wxz);
    TiledSum sum(tp, z_out);
    return tiled_batch<double>(tp, N, chains, class_out, [&](uint32_t group) { return sum.open(group); }, [](uint64_t, uint64_t) { return 0; },
                               [&](uint32_t unit_first, uint32_t units, const SweepBatch &b, double *work, double *P) {
                                   return launch_class_sweep_tiled(tp, wxz, unit_first, units, b.ops(), b.held(), b.rep(), work, P, 0);
                               },
                               [&](const SweepBatch &b, uint64_t first, uint64_t here, double *P) { return sum(b, first, here, P); });
}

// ---------------------------------------------------------------- the three sweeps under a weight per (syndrome, qubit) (class_sweep_site.hpp)
namespace {
// the host checks every site entry point makes once its sibling's plan is accepted: the rows, then every weight of a qubit some CLOSE names
int check_site(uint64_t N, const double *wq, uint64_t wq_rows, int nq, const std::vector<uint32_t> &ops)
{
    if (int rc = report(sweep::check_site_rows(N, wq_rows))) return rc;
    return N ? report(sweep::check_site_weights(wq, wq_rows, nq, sweep::closed_qubits(ops, nq))) : 0;
}

// The weight rows on the device, in (x, z) order: the one table once, or the rows of a launch group at a time -- `group` rows at most, whatever N.
struct SiteRows {
    DevBuf d;
    std::vector<double> host;
    const double *wq;
    size_t row;                                                                 // doubles of one row
    int nq, per_syndrome;
    int open(const double *wq_in, uint64_t wq_rows, int nq_in, uint32_t group)
    {
        wq = wq_in; nq = nq_in; row = (size_t)nq * 4u; per_syndrome = wq_rows != 1;
        host.resize((per_syndrome ? (size_t)group : 1u) * row);
        HIP_TRY(d.alloc(host.size() * sizeof(double)));
        if ((reinterpret_cast<uintptr_t>(d.p) & 31u) != 0) return fail(QECMC_ERR_HIP, "internal: the device block of the site weights is not 32-byte aligned");
        return per_syndrome ? 0 : upload(0, 1);
    }
    int upload(uint64_t first, uint64_t rows)
    {
        sweep::site_rows_xz(wq + first * row, rows, nq, host.data());
        HIP_TRY(hipMemcpy(d.p, host.data(), (size_t)rows * row * sizeof(double), hipMemcpyHostToDevice));
        return 0;
    }
    int group(uint64_t first, uint64_t here) { return per_syndrome ? upload(first, here) : 0; }
};
}  // namespace

int qecmc_class_sweep_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, double *z_out, int32_t *class_out)
{
    if (!chains || !wq || !z_out) return fail(QECMC_ERR_INVALID, "qecmc_class_sweep_site: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    const sweep::Plan p = sweep::build_plan(code, L);
    if (int rc = report(p.refusal)) return rc;
    if (int rc = check_site(N, wq, wq_rows, p.nq, p.ops)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    SweepBatch b(p, sweep::launch_group(N));
    DevBuf dz;
    SiteRows rows;
    if (int rc = b.open(p.ops, nullptr)) return rc;
    HIP_TRY(dz.alloc((size_t)b.group * p.ncls * sizeof(double)));
    if (int rc = rows.open(wq, wq_rows, p.nq, b.group)) return rc;
    SweepSiteArgs a = {};
    a.ncls = p.ncls; a.W = p.W; a.width = p.width; a.n_ops = p.n_ops; a.nq = p.nq; a.per_syndrome = rows.per_syndrome; a.scale = p.scale;
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {     // (the weight rows do not grow with the batch either)
        if (int rc = rows.group(first, here)) return rc;
        a.S = (uint32_t)here;
        HIP_TRY(launch_class_sweep_site(a, b.ops(), b.rep(), rows.d.as<double>(), dz.as<double>(), 0));
        return b.fetch(z_out, dz, first, here);
    });
}

int qecmc_class_sweep_cut_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int lds_width, double *z_out, int32_t *class_out)
{
    if (!chains || !wq || !z_out) return fail(QECMC_ERR_INVALID, "qecmc_class_sweep_cut_site: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    const sweep::Plan &p = cp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (int rc = check_site(N, wq, wq_rows, p.nq, p.ops)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if (class_sweep_cut_site_allow_lds(p.width) != hipSuccess)
        return fail(QECMC_ERR_UNSUPPORTED, "this device does not grant a workgroup the %u bytes of LDS a state vector of width %d takes", p.carve.bytes, p.width);
    SweepBatch b(p, sweep::cut_launch_group(N, p.ncls, cp.n_held));
    const size_t partials = (size_t)p.ncls << cp.n_held;                        // of one syndrome
    DevBuf dpart, dz;
    SiteRows rows;
    if (int rc = b.open(p.ops, &cp.held_words)) return rc;
    HIP_TRY(dpart.alloc((size_t)b.group * partials * sizeof(double)));          // kCutGridMax doubles at most; dirty: every partial is written before it is read
    HIP_TRY(dz.alloc((size_t)b.group * p.ncls * sizeof(double)));
    if (int rc = rows.open(wq, wq_rows, p.nq, b.group)) return rc;
    SweepSiteArgs a = {};
    a.ncls = p.ncls; a.W = p.W; a.width = p.width; a.n_ops = p.n_ops; a.n_held = cp.n_held; a.nq = p.nq; a.per_syndrome = rows.per_syndrome; a.scale = p.scale;
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {
        if (int rc = rows.group(first, here)) return rc;
        a.S = (uint32_t)here;
        HIP_TRY(launch_class_sweep_cut_site(a, b.ops(), b.held(), b.rep(), rows.d.as<double>(), dpart.as<double>(), dz.as<double>(), 0));
        return b.fetch(z_out, dz, first, here);
    });
}

int qecmc_class_sweep_tiled_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int hbm_width, int tile_width, double *z_out,
                                 int32_t *class_out)
{
    if (!chains || !wq || !z_out) return fail(QECMC_ERR_INVALID, "qecmc_class_sweep_tiled_site: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, hbm_width, tile_width);
    const sweep::Plan &p = tp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (int rc = check_site(N, wq, wq_rows, p.nq, tp.ops)) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    SiteRows rows;
    TiledSum sum(tp, z_out);
    return tiled_batch<double>(tp, N, chains, class_out, [&](uint32_t group) { const int rc = sum.open(group); return rc ? rc : rows.open(wq, wq_rows, p.nq, group); },
                               [&](uint64_t first, uint64_t here) { return rows.group(first, here); },
                               [&](uint32_t unit_first, uint32_t units, const SweepBatch &b, double *work, double *P) {
                                   return launch_class_sweep_tiled_site(tp, rows.per_syndrome, unit_first, units, b.ops(), b.held(), b.rep(), rows.d.as<double>(), work, P,
                                                                        0);
                               },
                               [&](const SweepBatch &b, uint64_t first, uint64_t here, double *P) { return sum(b, first, here, P); });
}

// ---------------------------------------------------------------- exact chains of every class: the traced sum-product sweep (class_sample.hpp)
namespace {
int class_sample_impl(const char *name, int code, int L, uint64_t N, const uint8_t *chains, const double *w, const double *wq, uint64_t wq_rows, int lds_width, uint64_t K,
                      uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out)
{
    const bool site = w == nullptr;
    if (!chains || (site && !wq) || !chain_out || !z_out || (mode == 1 && !class_out)) return fail(QECMC_ERR_INVALID, "%s: NULL buffer", name);
    if (int rc = report(sample::check_sample_args(name, N, K, first_syndrome, mode))) return rc;
    if (!site)
        if (int rc = report(sample::check_sample_weights(name, w))) return rc;
    const sample::SamplePlan sp = sample::build_sample_plan(code, L, lds_width, name);
    const sweep::CutPlan &cp = sp.cut;
    const sweep::Plan &p = cp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (site)
        if (int rc = report(sample::check_sample_site(name, N, wq, wq_rows, p))) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if ((site ? class_sweep_cut_site_allow_lds(p.width) : class_sweep_cut_allow_lds(p.width)) != hipSuccess || class_sample_allow_lds(p.width, site) != hipSuccess)
        return fail(QECMC_ERR_UNSUPPORTED, "%s: this device does not grant a workgroup the %u bytes of LDS a state vector of width %d takes", name, p.carve.bytes, p.width);
    const uint64_t job_bytes = sample::sample_bytes_per_job(sp);
    const sample::LaunchGroup g = sample::sample_launch_group(N, p.ncls, cp.n_held, K, job_bytes);
    SweepBatch b(p, g.syndromes);
    const size_t pairs = (size_t)g.syndromes * p.ncls, per_syndrome = mode ? 1u : (size_t)p.ncls, max_samples = (size_t)g.syndromes * per_syndrome * g.k_chunk;
    DevBuf dforget, dpart, dfold, dz, dcls, dspair, dsh, djob, drec, drecord, dchain;
    SiteRows rows;
    if (int rc = b.open(p.ops, &cp.held_words)) return rc;
    HIP_TRY(dforget.alloc(sp.forget_words.size() * sizeof(uint32_t)));
    HIP_TRY(dpart.alloc((pairs << cp.n_held) * sizeof(double)));                // dirty: every partial is written before it is read
    HIP_TRY(dfold.alloc((pairs << cp.n_held) * sizeof(double)));                // the copy the reduce folds: the pick reads the partials as they were
    HIP_TRY(dz.alloc(pairs * sizeof(double)));
    HIP_TRY(dcls.alloc(max_samples * sizeof(int32_t)));
    HIP_TRY(dspair.alloc(max_samples * sizeof(uint32_t)));
    HIP_TRY(dsh.alloc(max_samples * sizeof(uint32_t)));
    HIP_TRY(djob.alloc(pairs * sizeof(uint32_t)));
    HIP_TRY(drec.alloc(pairs * sizeof(uint32_t)));
    HIP_TRY(drecord.alloc((size_t)g.jobs * (size_t)job_bytes));                 // kSampleWorkspaceBytes at most; dirty: the walk reads what the record kernel wrote
    HIP_TRY(dchain.alloc(max_samples * (size_t)p.nq));
    HIP_TRY(hipMemcpy(dforget.p, sp.forget_words.data(), sp.forget_words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (site)
        if (int rc = rows.open(wq, wq_rows, p.nq, b.group)) return rc;
    SweepCutArgs ca = cut_args(p, cp.n_held);
    SweepSiteArgs sa = {};
    sa.ncls = p.ncls; sa.W = p.W; sa.width = p.width; sa.n_ops = p.n_ops; sa.n_held = cp.n_held; sa.nq = p.nq; sa.per_syndrome = site ? rows.per_syndrome : 0; sa.scale = p.scale;
    SampleArgs a = {};
    a.ncls = p.ncls; a.W = p.W; a.width = p.width; a.n_ops = p.n_ops; a.n_held = cp.n_held; a.n_forget = sp.n_forget; a.nq = p.nq; a.per_syndrome = sa.per_syndrome; a.mode = mode;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    if (!site) { sweep::weights_xz(w, ca.wxz); sweep::weights_xz(w, a.wxz); }
    const double *dwq = site ? rows.d.as<double>() : nullptr;
    std::vector<int32_t> cls_h(max_samples);
    std::vector<uint32_t> job_h(pairs), rec_h(pairs);
    std::vector<uint8_t> chain_h(max_samples * (size_t)p.nq);
    return b.run(N, chains, nullptr, [&](uint64_t first, uint64_t here) {
        if (site)
            if (int rc = rows.group(first, here)) return rc;
        ca.S = sa.S = (uint32_t)here;
        const size_t part_bytes = ((size_t)here * p.ncls << cp.n_held) * sizeof(double);
        if (site) HIP_TRY(launch_class_sweep_cut_site_partials(sa, b.ops(), b.held(), b.rep(), dwq, dpart.as<double>(), 0));
        else HIP_TRY(launch_class_sweep_cut_partials(ca, b.ops(), b.held(), b.rep(), dpart.as<double>(), 0));
        HIP_TRY(hipMemcpyAsync(dfold.p, dpart.p, part_bytes, hipMemcpyDeviceToDevice, 0));
        HIP_TRY(launch_class_sweep_reduce(ca, dfold.as<double>(), dz.as<double>(), 0));
        if (int rc = b.fetch(z_out, dz, first, here)) return rc;
        for (uint64_t s = 0; s < here; ++s)
            if (int rc = report(sample::check_sample_z(name, first + s, z_out + (first + s) * (uint64_t)p.ncls, p.ncls, mode))) return rc;
        a.syndrome0 = first_syndrome + (uint32_t)first;
        for (uint64_t k0 = 0; k0 < K; k0 += g.k_chunk) {
            const uint32_t kc = (uint32_t)(K - k0 < g.k_chunk ? K - k0 : g.k_chunk);
            a.k0 = (uint32_t)k0; a.k_chunk = kc; a.n_samples = (uint32_t)(here * per_syndrome * kc);
            HIP_TRY(launch_sample_pick(a, dpart.as<double>(), dz.as<double>(), dcls.as<int32_t>(), dspair.as<uint32_t>(), dsh.as<uint32_t>(), 0));
            if (mode) {
                HIP_TRY(hipMemcpy(cls_h.data(), dcls.p, (size_t)a.n_samples * sizeof(int32_t), hipMemcpyDeviceToHost));
                for (uint64_t s = 0; s < here; ++s) std::memcpy(class_out + (first + s) * K + k0, cls_h.data() + s * kc, (size_t)kc * sizeof(int32_t));
            }
            if (cp.n_held == 0) {                                               // a job per pair: every pair in mode 0, the drawn pairs in mode 1
                uint32_t jobs = 0;
                std::fill(rec_h.begin(), rec_h.end(), 0xFFFFFFFFu);
                if (mode) {
                    for (uint32_t i = 0; i < a.n_samples; ++i) {
                        const uint32_t pair = (i / kc) * (uint32_t)p.ncls + (uint32_t)cls_h[i];
                        if (pair >= pairs) return fail(QECMC_ERR_HIP, "%s: internal: sample %u drew a class outside the %d of the code", name, i, p.ncls);
                        if (rec_h[pair] == 0xFFFFFFFFu) { rec_h[pair] = jobs; job_h[jobs++] = pair; }
                    }
                } else
                    for (; jobs < (uint32_t)(here * p.ncls); ++jobs) rec_h[jobs] = job_h[jobs] = jobs;
                HIP_TRY(hipMemcpy(djob.p, job_h.data(), (size_t)jobs * sizeof(uint32_t), hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(drec.p, rec_h.data(), (size_t)here * p.ncls * sizeof(uint32_t), hipMemcpyHostToDevice));
                HIP_TRY(launch_sample_record(a, jobs, b.ops(), b.held(), b.rep(), dwq, djob.as<uint32_t>(), nullptr, drecord.as<sample::PairRecord>(), 0));
                HIP_TRY(launch_sample_walk(a, 0, a.n_samples, b.ops(), b.held(), b.rep(), dforget.as<uint32_t>(), dspair.as<uint32_t>(), dsh.as<uint32_t>(), drec.as<uint32_t>(),
                                           drecord.as<sample::PairRecord>(), jobs, dchain.as<uint8_t>(), 0));
            } else                                                              // a job per sample, as many at a time as the workspace holds records
                for (uint32_t j0 = 0; j0 < a.n_samples; j0 += g.jobs) {
                    const uint32_t jobs = a.n_samples - j0 < g.jobs ? a.n_samples - j0 : g.jobs;
                    HIP_TRY(launch_sample_record(a, jobs, b.ops(), b.held(), b.rep(), dwq, dspair.as<uint32_t>() + j0, dsh.as<uint32_t>() + j0, drecord.as<sample::PairRecord>(), 0));
                    HIP_TRY(launch_sample_walk(a, j0, jobs, b.ops(), b.held(), b.rep(), dforget.as<uint32_t>(), dspair.as<uint32_t>(), dsh.as<uint32_t>(), nullptr,
                                               drecord.as<sample::PairRecord>(), jobs, dchain.as<uint8_t>(), 0));
                }
            HIP_TRY(hipMemcpy(chain_h.data(), dchain.p, (size_t)a.n_samples * p.nq, hipMemcpyDeviceToHost));
            const size_t run = (size_t)kc * p.nq;                               // the kc chains of one (syndrome[, class]) are contiguous on both sides
            for (uint64_t r = 0; r < here * per_syndrome; ++r) std::memcpy(chain_out + ((first * per_syndrome + r) * K + k0) * (uint64_t)p.nq, chain_h.data() + r * run, run);
        }
        return 0;
    });
}
}  // namespace

int qecmc_class_sample(int code, int L, uint64_t N, const uint8_t *chains, const double w[4], int lds_width, uint64_t K, uint64_t seed, uint32_t first_syndrome, int mode,
                       uint8_t *chain_out, int32_t *class_out, double *z_out)
{
    if (!w) return fail(QECMC_ERR_INVALID, "qecmc_class_sample: NULL buffer");
    return class_sample_impl("qecmc_class_sample", code, L, N, chains, w, nullptr, 0, lds_width, K, seed, first_syndrome, mode, chain_out, class_out, z_out);
}

int qecmc_class_sample_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int lds_width, uint64_t K, uint64_t seed,
                            uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out)
{
    return class_sample_impl("qecmc_class_sample_site", code, L, N, chains, nullptr, wq, wq_rows, lds_width, K, seed, first_syndrome, mode, chain_out, class_out, z_out);
}

// ---------------------------------------------------------------- exact per-qubit marginals of every class: the backward sweep (class_marginal.hpp)
namespace {
int class_marginals_impl(const char *name, int code, int L, uint64_t N, const uint8_t *chains, const double *w, const double *wq, uint64_t wq_rows, int lds_width,
                         double *weights_out, double *z_out, int32_t *class_out)
{
    const bool site = w == nullptr;
    if (!chains || (site && !wq) || !weights_out || !z_out) return fail(QECMC_ERR_INVALID, "%s: NULL buffer", name);
    if (int rc = report(marginal::check_marginal_args(name, N))) return rc;
    if (!site)
        if (int rc = report(marginal::check_marginal_weights(name, w))) return rc;
    const marginal::MarginalPlan mp = marginal::build_marginal_plan(code, L, lds_width, name);
    const sweep::CutPlan &cp = mp.cut;
    const sweep::Plan &p = cp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (site)
        if (int rc = report(marginal::check_marginal_site(name, N, wq, wq_rows, p))) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if (class_marginal_allow_lds(p.width, site) != hipSuccess)
        return fail(QECMC_ERR_UNSUPPORTED, "%s: this device does not grant a workgroup the %u bytes of LDS a state vector of width %d takes", name, p.carve.bytes, p.width);
    const uint64_t job_bytes = marginal::marginal_bytes_per_job(mp);
    const marginal::LaunchGroup g = marginal::marginal_launch_group(N, p.ncls, cp.n_held, mp.n_close, job_bytes);
    SweepBatch b(p, g.syndromes);
    const size_t pairs = (size_t)g.syndromes * p.ncls, all_jobs = pairs << cp.n_held, row = (size_t)p.nq * 4u;
    DevBuf dclose, dcloseof, dpart, dz, dfwd, dmh, dout;
    SiteRows rows;
    if (int rc = b.open(p.ops, &cp.held_words)) return rc;
    HIP_TRY(dclose.alloc(mp.close_op.size() * sizeof(uint32_t)));
    HIP_TRY(dcloseof.alloc(mp.close_of.size() * sizeof(int32_t)));
    HIP_TRY(dpart.alloc(all_jobs * sizeof(double)));                            // kCutGridMax doubles at most; dirty: every partial is written before it is read
    HIP_TRY(dz.alloc(pairs * sizeof(double)));
    HIP_TRY(dfwd.alloc((size_t)g.jobs * (size_t)job_bytes));                    // kMarginalWorkspaceBytes at most; dirty: only live entries are written and read
    HIP_TRY(dmh.alloc(all_jobs * (size_t)marginal::marginal_fold_per_job(mp.n_close) * sizeof(double)));      // every row is written by the fold before the combine reads it
    HIP_TRY(dout.alloc(pairs * row * sizeof(double)));
    HIP_TRY(hipMemcpy(dclose.p, mp.close_op.data(), mp.close_op.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dcloseof.p, mp.close_of.data(), mp.close_of.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (site)
        if (int rc = rows.open(wq, wq_rows, p.nq, b.group)) return rc;
    SweepCutArgs ca = cut_args(p, cp.n_held);
    MarginalArgs a = {};
    a.ncls = p.ncls; a.W = p.W; a.width = p.width; a.n_ops = p.n_ops; a.n_held = cp.n_held; a.n_close = mp.n_close; a.nq = p.nq; a.per_syndrome = site ? rows.per_syndrome : 0;
    a.scale = p.scale;
    if (!site) sweep::weights_xz(w, a.wxz);
    const double *dwq = site ? rows.d.as<double>() : nullptr;
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {
        if (site)
            if (int rc = rows.group(first, here)) return rc;
        ca.S = a.S = (uint32_t)here;
        const uint32_t jobs_here = (uint32_t)(((size_t)here * p.ncls) << cp.n_held);
        for (uint32_t j0 = 0; j0 < jobs_here; j0 += g.jobs) {                   // as many jobs at a time as the workspace holds records
            a.job0 = j0; a.jobs = jobs_here - j0 < g.jobs ? jobs_here - j0 : g.jobs;
            HIP_TRY(launch_marginal_forward(a, b.ops(), b.held(), b.rep(), dwq, dfwd.as<double>(), dpart.as<double>(), 0));
            HIP_TRY(launch_marginal_backward(a, b.ops(), b.held(), b.rep(), dwq, dfwd.as<double>(), 0));
            HIP_TRY(launch_marginal_fold(a, b.ops(), b.held(), b.rep(), dclose.as<uint32_t>(), dfwd.as<double>(), dmh.as<double>(), 0));
        }
        HIP_TRY(launch_class_sweep_reduce(ca, dpart.as<double>(), dz.as<double>(), 0));
        HIP_TRY(launch_marginal_combine(a, b.rep(), dcloseof.as<int32_t>(), dmh.as<double>(), dz.as<double>(), dout.as<double>(), 0));
        if (int rc = b.fetch(z_out, dz, first, here)) return rc;
        return b.fetch(weights_out, dout, first, here, row);
    });
}
}  // namespace

int qecmc_class_marginals(int code, int L, uint64_t N, const uint8_t *chains, const double w[4], int lds_width, double *weights_out, double *z_out, int32_t *class_out)
{
    if (!w) return fail(QECMC_ERR_INVALID, "qecmc_class_marginals: NULL buffer");
    return class_marginals_impl("qecmc_class_marginals", code, L, N, chains, w, nullptr, 0, lds_width, weights_out, z_out, class_out);
}

int qecmc_class_marginals_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int lds_width, double *weights_out, double *z_out,
                               int32_t *class_out)
{
    return class_marginals_impl("qecmc_class_marginals_site", code, L, N, chains, nullptr, wq, wq_rows, lds_width, weights_out, z_out, class_out);
}

// ---------------------------------------------------------------- the (min, +) sweep and its traceback under a cost per (syndrome, qubit) (class_minplus_site.hpp)
namespace {
// The cost words on the device: the one table once, or the rows of a launch group at a time -- `group` rows at most, whatever N.
struct CostRows {
    DevBuf d;
    std::vector<uint32_t> host;
    const uint8_t *cq;
    int nq, per_syndrome;
    int open(const uint8_t *cq_in, uint64_t cq_rows, int nq_in, uint32_t group)
    {
        cq = cq_in; nq = nq_in; per_syndrome = cq_rows != 1;
        host.resize((per_syndrome ? (size_t)group : 1u) * (size_t)nq);
        HIP_TRY(d.alloc(host.size() * sizeof(uint32_t)));
        return per_syndrome ? 0 : upload(0, 1);
    }
    int upload(uint64_t first, uint64_t rows)
    {
        minplus::site_cost_words(cq + first * (uint64_t)nq * 4u, rows, nq, host.data());
        HIP_TRY(hipMemcpy(d.p, host.data(), (size_t)rows * (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice));
        return 0;
    }
    int group(uint64_t first, uint64_t here) { return per_syndrome ? upload(first, here) : 0; }
};

// every CLOSE of the stream names a cell of the table: the kernels index a row of nq words by it
bool closes_within(const std::vector<uint32_t> &ops, int nq)
{
    for (size_t o = 0; o + 3 < ops.size(); o += 4)
        if ((ops[o] & 15u) == sweep::kClose && ops[o + 3] >= (uint32_t)nq) return false;
    return true;
}
}  // namespace

int qecmc_class_minplus_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int lds_width, uint32_t *cost_out, uint64_t *count_out,
                             int32_t *class_out)
{
    if (!chains || !cq || !cost_out || !count_out) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_site: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_site: N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    const sweep::CutPlan cp = minplus::build_minplus_site_plan(code, L, lds_width);
    const sweep::Plan &p = cp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (int rc = report(minplus::check_cost_rows("qecmc_class_minplus_site", N, cq_rows))) return rc;
    if (!closes_within(p.ops, p.nq)) return fail(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_site: internal: a CLOSE names a cell beyond the %d of the table", p.nq);
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if (class_minplus_site_allow_lds(p.width) != hipSuccess)
        return fail(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_site: this device does not grant a workgroup the %u bytes of LDS a state vector of width %d takes",
                    p.carve.bytes, p.width);
    SweepBatch b(p, sweep::cut_launch_group(N, p.ncls, cp.n_held));
    const size_t partials = (size_t)p.ncls << cp.n_held;                        // of one syndrome
    DevBuf dpart, dcost, dcount;
    CostRows rows;
    if (int rc = b.open(p.ops, &cp.held_words)) return rc;
    HIP_TRY(dpart.alloc((size_t)b.group * partials * sizeof(uint64_t)));        // kCutGridMax entries at most; dirty: every partial is written before it is read
    HIP_TRY(dcost.alloc((size_t)b.group * p.ncls * sizeof(uint32_t)));
    HIP_TRY(dcount.alloc((size_t)b.group * p.ncls * sizeof(uint64_t)));
    if (int rc = rows.open(cq, cq_rows, p.nq, b.group)) return rc;
    MinplusSiteArgs sa = {};
    MinplusArgs &a = sa.t.m;
    a = minplus_args(p, cp.n_held);
    sa.t.nq = p.nq; sa.per_syndrome = rows.per_syndrome;
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {     // (the cost rows do not grow with the batch either)
        if (int rc = rows.group(first, here)) return rc;
        a.S = (uint32_t)here;
        HIP_TRY(launch_class_minplus_site_sweep(sa, b.ops(), b.held(), b.rep(), rows.d.as<uint32_t>(), dpart.as<uint64_t>(), 0));
        HIP_TRY(launch_class_minplus_reduce(a, dpart.as<uint64_t>(), dcost.as<uint32_t>(), dcount.as<uint64_t>(), 0));
        if (int rc = b.fetch(cost_out, dcost, first, here)) return rc;
        return b.fetch(count_out, dcount, first, here);
    });
}

int qecmc_class_minplus_chains_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int lds_width, uint8_t *chain_out,
                                    uint32_t *cost_out, uint64_t *count_out, int32_t *class_out)
{
    if (!chains || !cq || !chain_out) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_chains_site: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_chains_site: N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    const minplus::TracePlan tp = minplus::build_trace_site_plan(code, L, lds_width);
    const sweep::CutPlan &cp = tp.cut;
    const sweep::Plan &p = cp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (int rc = report(minplus::check_cost_rows("qecmc_class_minplus_chains_site", N, cq_rows))) return rc;
    if (!closes_within(p.ops, p.nq)) return fail(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_chains_site: internal: a CLOSE names a cell beyond the %d of the table", p.nq);
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    if (class_minplus_site_allow_lds(p.width) != hipSuccess || class_minplus_trace_site_allow_lds(p.width) != hipSuccess)
        return fail(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_chains_site: this device does not grant a workgroup the %u bytes of LDS a state vector of width %d takes",
                    p.carve.bytes, p.width);
    const uint64_t pair_bytes = minplus::trace_bytes_per_pair(tp);
    SweepBatch b(p, minplus::trace_launch_group(N, p.ncls, cp.n_held, pair_bytes));
    TraceBlocks d;
    CostRows rows;
    if (int rc = b.open(p.ops, &cp.held_words)) return rc;
    if (int rc = d.open(b, tp, pair_bytes)) return rc;
    if (int rc = rows.open(cq, cq_rows, p.nq, b.group)) return rc;
    MinplusSiteArgs sa = {};
    MinplusTraceArgs &t = sa.t;
    MinplusArgs &a = t.m;
    a = minplus_args(p, cp.n_held);
    t.n_forget = tp.n_forget; t.words_per_forget = tp.words_per_forget; t.nq = p.nq;
    sa.per_syndrome = rows.per_syndrome;
    return b.run(N, chains, class_out, [&](uint64_t first, uint64_t here) {     // (the cost rows do not grow with the batch either)
        if (int rc = rows.group(first, here)) return rc;
        a.S = (uint32_t)here;
        HIP_TRY(launch_class_minplus_site_sweep(sa, b.ops(), b.held(), b.rep(), rows.d.as<uint32_t>(), d.dpart.as<uint64_t>(), 0));
        HIP_TRY(launch_minplus_pick(a, d.dpart.as<uint64_t>(), d.dpick.as<uint32_t>(), 0));          // (before the reduce folds the partials in place)
        HIP_TRY(launch_class_minplus_reduce(a, d.dpart.as<uint64_t>(), d.dcost.as<uint32_t>(), d.dcount.as<uint64_t>(), 0));
        HIP_TRY(launch_minplus_trace_site(sa, b.ops(), b.held(), b.rep(), rows.d.as<uint32_t>(), d.dpick.as<uint32_t>(), d.ddec.as<uint64_t>(), 0));
        HIP_TRY(launch_minplus_walk(t, b.ops(), b.held(), b.rep(), d.dforget.as<uint32_t>(), d.dpick.as<uint32_t>(), d.ddec.as<uint64_t>(), d.dchain.as<uint8_t>(), 0));
        return d.fetch(b, first, here, chain_out, cost_out, count_out);
    });
}

// ---------------------------------------------------------------- the (min, +) sweep on the state vector tiled over HBM (class_minplus_tiled.hpp)
int qecmc_class_minplus_tiled(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t cost[4], int hbm_width, int tile_width, uint32_t *cost_out,
                              uint64_t *count_out, int32_t *class_out)
{
    if (!chains || !cost || !cost_out || !count_out) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled: N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    if (int rc = report(minplus::check_tiled_costs(cost))) return rc;
    const sweep::TiledPlan tp = minplus::build_minplus_tiled_plan(code, L, hbm_width, tile_width, "qecmc_class_minplus_tiled");
    if (int rc = report(tp.plan.refusal)) return rc;
    if (int rc = report(minplus::check_tiled_cost_range(tp.plan, cost))) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    uint32_t cxz[4];
    minplus::costs_xz(cost, cxz);
    TiledFold fold(tp, cost_out, count_out);
    return tiled_batch<uint64_t>(tp, N, chains, class_out, [&](uint32_t group) { return fold.open(group); }, [](uint64_t, uint64_t) { return 0; },
                                 [&](uint32_t unit_first, uint32_t units, const SweepBatch &b, uint64_t *work, uint64_t *P) {
                                     return launch_class_minplus_tiled(tp, cxz, unit_first, units, b.ops(), b.held(), b.rep(), work, P, 0);
                                 },
                                 [&](const SweepBatch &b, uint64_t first, uint64_t here, uint64_t *P) { return fold(b, first, here, P); });
}

int qecmc_class_minplus_tiled_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int hbm_width, int tile_width, uint32_t *cost_out,
                                   uint64_t *count_out, int32_t *class_out)
{
    if (!chains || !cq || !cost_out || !count_out) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled_site: NULL buffer");
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled_site: N=%llu syndromes exceed 32 bits", (unsigned long long)N);
    const sweep::TiledPlan tp = minplus::build_minplus_tiled_plan(code, L, hbm_width, tile_width, "qecmc_class_minplus_tiled_site");
    const sweep::Plan &p = tp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (int rc = report(minplus::check_cost_rows("qecmc_class_minplus_tiled_site", N, cq_rows))) return rc;
    if (!closes_within(tp.ops, p.nq)) return fail(QECMC_ERR_UNSUPPORTED, "qecmc_class_minplus_tiled_site: internal: a CLOSE names a cell beyond the %d of the table", p.nq);
    if (N > 0)
        if (int rc = report(minplus::check_tiled_cost_rows_range(cq, cq_rows, p.nq, sweep::closed_qubits(tp.ops, p.nq)))) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    CostRows rows;
    TiledFold fold(tp, cost_out, count_out);
    return tiled_batch<uint64_t>(tp, N, chains, class_out, [&](uint32_t group) { const int rc = fold.open(group); return rc ? rc : rows.open(cq, cq_rows, p.nq, group); },
                                 [&](uint64_t first, uint64_t here) { return rows.group(first, here); },
                                 [&](uint32_t unit_first, uint32_t units, const SweepBatch &b, uint64_t *work, uint64_t *P) {
                                     return launch_class_minplus_tiled_site(tp, rows.per_syndrome, unit_first, units, b.ops(), b.held(), b.rep(), rows.d.as<uint32_t>(), work,
                                                                            P, 0);
                                 },
                                 [&](const SweepBatch &b, uint64_t first, uint64_t here, uint64_t *P) { return fold(b, first, here, P); });
}

// ---------------------------------------------------------------- a shortest chain per class on the tiled route (class_minplus_tiled_trace.hpp)
namespace {
// The decision words of one trace pass: one block per device, taken when a traced call first needs more than is there and kept --
// kTiledTraceWorkspaceBytes at most, never cleared.  Only the traced entry points touch it, and only while they hold the tiled workspace's lock.
struct TiledTraceBlock {
    void *p[TiledWorkspace::kDevices] = {};
    size_t bytes[TiledWorkspace::kDevices] = {};
    static TiledTraceBlock &get() { static TiledTraceBlock *b = new TiledTraceBlock; return *b; }   // (never destroyed, as DevPool)
    hipError_t take(size_t want, void **out)                                      // under TiledWorkspace::mu
    {
        int dev = 0;
        if (hipError_t e = hipGetDevice(&dev)) return e;
        if (dev < 0 || dev >= TiledWorkspace::kDevices || want > minplus::kTiledTraceWorkspaceBytes) return hipErrorInvalidValue;
        if (bytes[dev] < want) {
            if (p[dev]) { (void)hipFree(p[dev]); p[dev] = nullptr; bytes[dev] = 0; }
            if (hipError_t e = hipMalloc(&p[dev], want)) return e;
            bytes[dev] = want;
        }
        *out = p[dev];
        return hipSuccess;
    }
};

// both traced entry points: cost (the four costs) or cq (a site table).  Per group of syndromes: the sweep passes of qecmc_class_minplus_tiled(_site),
// the pick, the reduce, then trace passes of pairs -- as many as the state workspace and the decision block take -- each ending with its walk.
int tiled_chains_impl(const char *name, int code, int L, uint64_t N, const uint8_t *chains, const uint32_t *cost, const uint8_t *cq, uint64_t cq_rows, int hbm_width,
                      int tile_width, uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out, int32_t *class_out)
{
    if (!chains || (!cost && !cq) || !chain_out) return fail(QECMC_ERR_INVALID, "%s: NULL buffer", name);
    if (N > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "%s: N=%llu syndromes exceed 32 bits", name, (unsigned long long)N);
    if (cost)
        if (int rc = report(minplus::check_tiled_chain_costs(nullptr, cost))) return rc;
    const minplus::TiledTracePlan ttp = minplus::build_tiled_trace_plan(code, L, hbm_width, tile_width, name);
    const sweep::TiledPlan &tp = ttp.tiled;
    const sweep::Plan &p = tp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (cost) {
        if (int rc = report(minplus::check_tiled_chain_costs(&p, cost))) return rc;
    } else {
        if (int rc = report(minplus::check_cost_rows(name, N, cq_rows))) return rc;
        if (!closes_within(tp.ops, p.nq)) return fail(QECMC_ERR_UNSUPPORTED, "%s: internal: a CLOSE names a cell beyond the %d of the table", name, p.nq);
        if (N > 0)
            if (int rc = report(minplus::check_tiled_chain_cost_rows_range(cq, cq_rows, p.nq, sweep::closed_qubits(tp.ops, p.nq)))) return rc;
    }
    if (p.W > 64) return fail(QECMC_ERR_UNSUPPORTED, "%s: internal: a chain of %d state words does not fit the lanes of the walk", name, p.W);
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    uint32_t cxz[4] = {0, 0, 0, 0};
    if (cost) minplus::costs_xz(cost, cxz);
    CostRows rows;
    TiledFold fold(tp, cost_out, count_out);
    DevBuf dwide, dftile, dfwords, dpick, dchain;
    MinplusArgs pa = minplus_args(p, tp.n_held);
    pa.width = tp.tile_width;                                                   // (k_minplus_pick reads n_held alone; its launch asks for a width an LDS vector has)
    const uint64_t pair_bytes = minplus::tiled_trace_bytes_per_pair(ttp);
    uint64_t *work = nullptr;                                                   // the state workspace, as the sweep passes of the call were handed it
    return tiled_batch<uint64_t>(
        tp, N, chains, class_out,
        [&](uint32_t group) {
            const size_t pairs = (size_t)group * p.ncls;
            if (int rc = fold.open(group)) return rc;
            if (cq)
                if (int rc = rows.open(cq, cq_rows, p.nq, group)) return rc;
            HIP_TRY(dwide.alloc(tp.ops.size() * sizeof(uint32_t)));
            HIP_TRY(dftile.alloc(ttp.forget_tile.size() * sizeof(uint32_t)));
            HIP_TRY(dfwords.alloc(ttp.forget_words.size() * sizeof(uint32_t)));
            HIP_TRY(dpick.alloc(pairs * sizeof(uint32_t)));
            HIP_TRY(dchain.alloc(pairs * (size_t)p.nq));
            HIP_TRY(hipMemcpy(dwide.p, tp.ops.data(), tp.ops.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dftile.p, ttp.forget_tile.data(), ttp.forget_tile.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dfwords.p, ttp.forget_words.data(), ttp.forget_words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            return 0;
        },
        [&](uint64_t first, uint64_t here) { return cq ? rows.group(first, here) : 0; },
        [&](uint32_t unit_first, uint32_t units, const SweepBatch &b, uint64_t *w, uint64_t *P) {
            work = w;
            return cq ? launch_class_minplus_tiled_site(tp, rows.per_syndrome, unit_first, units, b.ops(), b.held(), b.rep(), rows.d.as<uint32_t>(), w, P, 0)
                      : launch_class_minplus_tiled(tp, cxz, unit_first, units, b.ops(), b.held(), b.rep(), w, P, 0);
        },
        [&](const SweepBatch &b, uint64_t first, uint64_t here, uint64_t *P) {
            pa.S = (uint32_t)here;
            HIP_TRY(launch_minplus_pick(pa, P, dpick.as<uint32_t>(), 0));         // (before the reduce folds the partials in place)
            if (int rc = fold(b, first, here, P)) return rc;
            const uint64_t pairs = here * (uint64_t)p.ncls;
            void *dec = nullptr;
            HIP_TRY(TiledTraceBlock::get().take((size_t)(minplus::tiled_trace_pass_pairs(tp.state_bits, pair_bytes, pairs) * pair_bytes), &dec));
            for (uint64_t first_pair = 0; first_pair < pairs;) {
                const uint32_t n = minplus::tiled_trace_pass_pairs(tp.state_bits, pair_bytes, pairs - first_pair);
                HIP_TRY(launch_minplus_tiled_trace(ttp, cq ? nullptr : cxz, cq ? rows.per_syndrome : 0, (uint32_t)first_pair, n, b.ops(), dwide.as<uint32_t>(), b.held(), b.rep(),
                                                   cq ? rows.d.as<uint32_t>() : nullptr, dpick.as<uint32_t>(), dftile.as<uint32_t>(), dfwords.as<uint32_t>(), work,
                                                   static_cast<uint64_t *>(dec), dchain.as<uint8_t>(), 0));
                first_pair += n;
            }
            return b.fetch(chain_out, dchain, first, here, (size_t)p.nq);
        });
}
}  // namespace

int qecmc_class_minplus_tiled_chains(int code, int L, uint64_t N, const uint8_t *chains, const uint32_t cost[4], int hbm_width, int tile_width, uint8_t *chain_out,
                                     uint32_t *cost_out, uint64_t *count_out, int32_t *class_out)
{
    if (!cost) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled_chains: NULL buffer");
    return tiled_chains_impl("qecmc_class_minplus_tiled_chains", code, L, N, chains, cost, nullptr, 0, hbm_width, tile_width, chain_out, cost_out, count_out, class_out);
}

int qecmc_class_minplus_tiled_chains_site(int code, int L, uint64_t N, const uint8_t *chains, const uint8_t *cq, uint64_t cq_rows, int hbm_width, int tile_width,
                                          uint8_t *chain_out, uint32_t *cost_out, uint64_t *count_out, int32_t *class_out)
{
    if (!cq) return fail(QECMC_ERR_INVALID, "qecmc_class_minplus_tiled_chains_site: NULL buffer");
    return tiled_chains_impl("qecmc_class_minplus_tiled_chains_site", code, L, N, chains, nullptr, cq, cq_rows, hbm_width, tile_width, chain_out, cost_out, count_out, class_out);
}

// ---------------------------------------------------------------- exact chains of every class on the tiled route (class_sample_tiled.hpp)
namespace {
static_assert(sample::kTiledLaunchSamples == sample::kLaunchSamples, "the pick of class_sample.hip serves both routes");

// The records of one record pass: one block per device, taken when a call first needs more than is there and kept up to kTiledSampleRecordBytes; a
// block a raised cap grew past that is freed when the call ends (Trim).  Never cleared.  Only the tiled sampler touches it, and only while it holds
// the tiled workspace's lock.
struct TiledSampleBlock {
    void *p[TiledWorkspace::kDevices] = {};
    size_t bytes[TiledWorkspace::kDevices] = {};
    static TiledSampleBlock &get() { static TiledSampleBlock *b = new TiledSampleBlock; return *b; }   // (never destroyed, as DevPool)
    hipError_t take(size_t want, uint64_t cap, void **out)                        // under TiledWorkspace::mu
    {
        int dev = 0;
        if (hipError_t e = hipGetDevice(&dev)) return e;
        if (dev < 0 || dev >= TiledWorkspace::kDevices || want > cap || cap > sample::kTiledSampleRecordBytesMax) return hipErrorInvalidValue;
        if (bytes[dev] < want) {
            if (p[dev]) { (void)hipFree(p[dev]); p[dev] = nullptr; bytes[dev] = 0; }
            if (hipError_t e = hipMalloc(&p[dev], want)) return e;
            bytes[dev] = want;
        }
        *out = p[dev];
        return hipSuccess;
    }
    struct Trim {                                                                 // under TiledWorkspace::mu: declared after the lock, so it runs before the unlock
        ~Trim()
        {
            TiledSampleBlock &b = TiledSampleBlock::get();
            int dev = 0;
            if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= TiledWorkspace::kDevices) return;
            if (b.bytes[dev] > sample::kTiledSampleRecordBytes) { (void)hipFree(b.p[dev]); b.p[dev] = nullptr; b.bytes[dev] = 0; }
        }
    };
};

// both entry points: w (the four weights) or wq (a site table).  Per group of syndromes: the sweep passes of qecmc_class_sweep_tiled(_site) with the
// partials left unfolded, the reduce on a copy, the checks Z decides; then per chunk of samples the pick of class_sample.hip and record passes of
// jobs -- as many as the state workspace and the record block take -- each ending with the walk of its samples.
int class_sample_tiled_impl(const char *name, int code, int L, uint64_t N, const uint8_t *chains, const double *w, const double *wq, uint64_t wq_rows, int hbm_width,
                            int tile_width, uint64_t record_bytes, uint64_t K, uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out,
                            double *z_out)
{
    const bool site = w == nullptr;
    if (!chains || (site && !wq) || !chain_out || !z_out || (mode == 1 && !class_out)) return fail(QECMC_ERR_INVALID, "%s: NULL buffer", name);
    if (int rc = report(sample::check_sample_args(name, N, K, first_syndrome, mode))) return rc;
    if (!site)
        if (int rc = report(sample::check_sample_weights(name, w))) return rc;
    uint64_t cap = 0;
    if (int rc = report(sample::check_record_bytes(name, record_bytes, &cap))) return rc;
    const sample::TiledSamplePlan tsp = sample::build_tiled_sample_plan(code, L, hbm_width, tile_width, name, cap);
    const sweep::TiledPlan &tp = tsp.tiled;
    const sweep::Plan &p = tp.plan;
    if (int rc = report(p.refusal)) return rc;
    if (site)
        if (int rc = report(sample::check_sample_tiled_site(name, N, wq, wq_rows, tp))) return rc;
    if (int rc = use_device(0)) return rc;
    if (N == 0) return 0;
    const uint64_t job_bytes = sample::tiled_sample_bytes_per_job(tsp);
    const uint32_t pass = sweep::tiled_pass_units(tp.state_bits);
    const size_t partials = (size_t)p.ncls << tp.n_held, per_syndrome = mode ? 1u : (size_t)p.ncls;
    SweepBatch b(p, sweep::cut_launch_group(N, p.ncls, tp.n_held));
    uint64_t kc_max = sample::kTiledLaunchSamples / ((uint64_t)b.group * (uint64_t)p.ncls);
    if (kc_max < 1ull) kc_max = 1ull;
    const uint32_t k_chunk = (uint32_t)(K < kc_max ? K : kc_max);
    const size_t pairs = (size_t)b.group * p.ncls, max_samples = (size_t)b.group * per_syndrome * k_chunk;
    const uint64_t group_units = (uint64_t)b.group * partials, max_jobs = tp.n_held == 0 ? (uint64_t)pairs : (uint64_t)max_samples;
    DevBuf dwide, dftile, dfwords, dpart, dfold, dz, dcls, dspair, dsh, djob, drec, dchain;
    SiteRows rows;
    if (int rc = b.open(tp.dev_ops, &tp.held_words)) return rc;
    HIP_TRY(dwide.alloc(tp.ops.size() * sizeof(uint32_t)));
    HIP_TRY(dftile.alloc(tsp.forget_tile.size() * sizeof(uint32_t)));
    HIP_TRY(dfwords.alloc(tsp.forget_words.size() * sizeof(uint32_t)));
    HIP_TRY(dpart.alloc((size_t)group_units * sizeof(double)));                 // kCutGridMax doubles at most; dirty: every partial is written before it is read
    HIP_TRY(dfold.alloc((size_t)group_units * sizeof(double)));                 // the copy the reduce folds: the pick reads the partials as they were
    HIP_TRY(dz.alloc(pairs * sizeof(double)));
    HIP_TRY(dcls.alloc(max_samples * sizeof(int32_t)));
    HIP_TRY(dspair.alloc(max_samples * sizeof(uint32_t)));
    HIP_TRY(dsh.alloc(max_samples * sizeof(uint32_t)));
    HIP_TRY(djob.alloc(pairs * sizeof(uint32_t)));
    HIP_TRY(drec.alloc(pairs * sizeof(uint32_t)));
    HIP_TRY(dchain.alloc(max_samples * (size_t)p.nq));
    HIP_TRY(hipMemcpy(dwide.p, tp.ops.data(), tp.ops.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dftile.p, tsp.forget_tile.data(), tsp.forget_tile.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dfwords.p, tsp.forget_words.data(), tsp.forget_words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (site)
        if (int rc = rows.open(wq, wq_rows, p.nq, b.group)) return rc;
    double wxz[4] = {0.0, 0.0, 0.0, 0.0};
    if (!site) sweep::weights_xz(w, wxz);
    const double *dwq = site ? rows.d.as<double>() : nullptr;
    SweepCutArgs ra = cut_args(p, tp.n_held);                                   // k_class_sweep_reduce's
    SampleArgs pa = {};                                                         // k_class_sample_pick's: it reads the counts, the mode, the holds and the draws' address alone
    pa.ncls = p.ncls; pa.n_held = tp.n_held; pa.mode = mode;
    pa.seed_lo = (uint32_t)seed; pa.seed_hi = (uint32_t)(seed >> 32);
    SampleTiledWalkArgs wa = {};
    wa.ncls = p.ncls; wa.W = p.W; wa.n_held = tp.n_held; wa.n_ops = p.n_ops; wa.n_forget = tsp.n_forget; wa.nq = p.nq; wa.tile_width = tp.tile_width;
    wa.seed_lo = pa.seed_lo; wa.seed_hi = pa.seed_hi; wa.pairs_per_job = tsp.pairs_per_job;
    std::vector<int32_t> cls_h(max_samples);
    std::vector<uint32_t> job_h(pairs), rec_h(pairs);
    std::vector<uint8_t> chain_h(max_samples * (size_t)p.nq);
    TiledWorkspace &ws = TiledWorkspace::get();                                 // the state vectors: the tiled sweeps' block, cap and lock
    std::lock_guard<std::mutex> hold(ws.mu);
    TiledSampleBlock::Trim trim;
    void *work_p = nullptr;
    const uint64_t most = group_units > max_jobs ? group_units : max_jobs;
    HIP_TRY(ws.take((size_t)(most < pass ? most : pass) * (sizeof(double) << tp.state_bits), &work_p));
    double *work = static_cast<double *>(work_p);
    return b.run(N, chains, nullptr, [&](uint64_t first, uint64_t here) {
        if (site)
            if (int rc = rows.group(first, here)) return rc;
        const uint64_t units = here * partials;
        for (uint64_t u = 0; u < units; u += pass) {
            const uint32_t n = (uint32_t)(units - u < pass ? units - u : pass);
            if (site) HIP_TRY(launch_class_sweep_tiled_site(tp, rows.per_syndrome, (uint32_t)u, n, b.ops(), b.held(), b.rep(), dwq, work, dpart.as<double>(), 0));
            else HIP_TRY(launch_class_sweep_tiled(tp, wxz, (uint32_t)u, n, b.ops(), b.held(), b.rep(), work, dpart.as<double>(), 0));
        }
        HIP_TRY(hipMemcpyAsync(dfold.p, dpart.p, (size_t)units * sizeof(double), hipMemcpyDeviceToDevice, 0));
        ra.S = (uint32_t)here;
        HIP_TRY(launch_class_sweep_reduce(ra, dfold.as<double>(), dz.as<double>(), 0));
        if (int rc = b.fetch(z_out, dz, first, here)) return rc;
        for (uint64_t s = 0; s < here; ++s)
            if (int rc = report(sample::check_sample_z(name, first + s, z_out + (first + s) * (uint64_t)p.ncls, p.ncls, mode))) return rc;
        pa.syndrome0 = wa.syndrome0 = first_syndrome + (uint32_t)first;
        for (uint64_t k0 = 0; k0 < K; k0 += k_chunk) {
            const uint32_t kc = (uint32_t)(K - k0 < k_chunk ? K - k0 : k_chunk);
            pa.k0 = wa.k0 = (uint32_t)k0; pa.k_chunk = wa.k_chunk = kc; pa.n_samples = (uint32_t)(here * per_syndrome * kc);
            HIP_TRY(launch_sample_pick(pa, dpart.as<double>(), dz.as<double>(), dcls.as<int32_t>(), dspair.as<uint32_t>(), dsh.as<uint32_t>(), 0));
            if (mode) {
                HIP_TRY(hipMemcpy(cls_h.data(), dcls.p, (size_t)pa.n_samples * sizeof(int32_t), hipMemcpyDeviceToHost));
                for (uint64_t s = 0; s < here; ++s) std::memcpy(class_out + (first + s) * K + k0, cls_h.data() + s * kc, (size_t)kc * sizeof(int32_t));
            }
            uint32_t jobs = 0;
            const uint32_t *job_pair = dspair.as<uint32_t>(), *job_hbits = dsh.as<uint32_t>(), *rec_of_pair = nullptr;      // a job per sample
            if (tp.n_held == 0) {                                               // a job per pair: every pair in mode 0, the drawn pairs in mode 1
                std::fill(rec_h.begin(), rec_h.end(), 0xFFFFFFFFu);
                if (mode) {
                    for (uint32_t i = 0; i < pa.n_samples; ++i) {
                        const uint32_t pair = (i / kc) * (uint32_t)p.ncls + (uint32_t)cls_h[i];
                        if (cls_h[i] < 0 || cls_h[i] >= p.ncls) return fail(QECMC_ERR_HIP, "%s: internal: sample %u drew a class outside the %d of the code", name, i, p.ncls);
                        if (rec_h[pair] == 0xFFFFFFFFu) { rec_h[pair] = jobs; job_h[jobs++] = pair; }
                    }
                } else
                    for (; jobs < (uint32_t)(here * p.ncls); ++jobs) rec_h[jobs] = job_h[jobs] = jobs;
                HIP_TRY(hipMemcpy(djob.p, job_h.data(), (size_t)jobs * sizeof(uint32_t), hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(drec.p, rec_h.data(), (size_t)here * p.ncls * sizeof(uint32_t), hipMemcpyHostToDevice));
                job_pair = djob.as<uint32_t>(); job_hbits = nullptr; rec_of_pair = drec.as<uint32_t>();
            } else
                jobs = pa.n_samples;
            void *rec_p = nullptr;
            HIP_TRY(TiledSampleBlock::get().take((size_t)(sample::tiled_sample_pass_jobs(tp.state_bits, job_bytes, jobs, cap) * job_bytes), cap, &rec_p));
            sample::PairRecord *R = static_cast<sample::PairRecord *>(rec_p);
            for (uint32_t j0 = 0; j0 < jobs;) {
                const uint32_t n = sample::tiled_sample_pass_jobs(tp.state_bits, job_bytes, jobs - j0, cap);
                HIP_TRY(launch_sample_tiled_record(tsp, site ? nullptr : wxz, site ? rows.per_syndrome : 0, j0, n, b.ops(), b.held(), b.rep(), dwq, job_pair, job_hbits,
                                                   dftile.as<uint32_t>(), work, R, 0));
                // the samples of the pass: contiguous where a job is a sample, or a pair in every-class mode ([s][c][kk]); every sample of the chunk in
                // posterior mode, where those of another pass leave at once
                wa.rec_first = j0; wa.records = n;
                if (tp.n_held > 0) { wa.first = j0; wa.count = n; }
                else if (mode == 0) { wa.first = j0 * kc; wa.count = n * kc; }
                else { wa.first = 0; wa.count = pa.n_samples; }
                HIP_TRY(launch_sample_tiled_walk(tsp, wa, dwide.as<uint32_t>(), b.held(), b.rep(), dfwords.as<uint32_t>(), dftile.as<uint32_t>(), dspair.as<uint32_t>(),
                                                 dsh.as<uint32_t>(), rec_of_pair, R, dchain.as<uint8_t>(), 0));
                j0 += n;
            }
            HIP_TRY(hipMemcpy(chain_h.data(), dchain.p, (size_t)pa.n_samples * p.nq, hipMemcpyDeviceToHost));
            const size_t run = (size_t)kc * p.nq;                               // the kc chains of one (syndrome[, class]) are contiguous on both sides
            for (uint64_t r = 0; r < here * per_syndrome; ++r) std::memcpy(chain_out + ((first * per_syndrome + r) * K + k0) * (uint64_t)p.nq, chain_h.data() + r * run, run);
        }
        return 0;
    });
}
}  // namespace

int qecmc_class_sample_tiled(int code, int L, uint64_t N, const uint8_t *chains, const double w[4], int hbm_width, int tile_width, uint64_t record_bytes, uint64_t K,
                             uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out)
{
    if (!w) return fail(QECMC_ERR_INVALID, "qecmc_class_sample_tiled: NULL buffer");
    return class_sample_tiled_impl("qecmc_class_sample_tiled", code, L, N, chains, w, nullptr, 0, hbm_width, tile_width, record_bytes, K, seed, first_syndrome, mode, chain_out,
                                   class_out, z_out);
}

int qecmc_class_sample_tiled_site(int code, int L, uint64_t N, const uint8_t *chains, const double *wq, uint64_t wq_rows, int hbm_width, int tile_width, uint64_t record_bytes,
                                  uint64_t K, uint64_t seed, uint32_t first_syndrome, int mode, uint8_t *chain_out, int32_t *class_out, double *z_out)
{
    return class_sample_tiled_impl("qecmc_class_sample_tiled_site", code, L, N, chains, nullptr, wq, wq_rows, hbm_width, tile_width, record_bytes, K, seed, first_syndrome, mode,
                                   chain_out, class_out, z_out);
}

int qecmc_class_sample_tiled_info(int code, int L, int hbm_width, int tile_width, uint64_t record_bytes, int32_t *n_forget, uint64_t *bytes_per_job, uint32_t *jobs_per_pass)
{
    uint64_t cap = 0;
    if (int rc = report(sample::check_record_bytes("qecmc_class_sample_tiled_info", record_bytes, &cap))) return rc;
    const sample::TiledSamplePlan tsp = sample::build_tiled_sample_plan(code, L, hbm_width, tile_width, "qecmc_class_sample_tiled_info", cap);
    if (tsp.n_forget > 0) {                                                     // (a plan refused for the cap alone has its tables)
        if (n_forget) *n_forget = tsp.n_forget;
        if (bytes_per_job) *bytes_per_job = sample::tiled_sample_bytes_per_job(tsp);
    }
    if (int rc = report(tsp.tiled.plan.refusal)) return rc;
    if (jobs_per_pass) *jobs_per_pass = sample::tiled_sample_pass_jobs(tsp.tiled.state_bits, sample::tiled_sample_bytes_per_job(tsp), ~0ull, cap);
    return 0;
}

// ---------------------------------------------------------------- chain / ladder
// (the drop-in calls gather their small buffers into one host block -- per thread, kept between calls -- and move it with one copy each way)
static std::vector<uint8_t> &staging()
{
    static thread_local std::vector<uint8_t> h;
    return h;
}
// (a large batch through these entry points must not leave its host copy behind in the thread)
struct StagingTrim {
    ~StagingTrim() { std::vector<uint8_t> &h = staging(); if (h.capacity() > (size_t(8) << 20)) std::vector<uint8_t>().swap(h); }
};

static int chain_update_impl(int code, int L, uint64_t N, uint8_t *states_inout, double p, double eta, int noise,
                             double p_logical, uint64_t iters, uint64_t seed, uint32_t first_syndrome, uint32_t slot, uint64_t k0,
                             uint8_t *accepted_out = nullptr)
{
    PRIM_PROLOGUE();
    if (!states_inout) return fail(QECMC_ERR_INVALID, "NULL buffer");
    if (noise == QECMC_NOISE_ALPHA) {      // `eta` carries alpha here
        if (!(p > 0.0) || !(p <= 1.0) || !(eta > 0.0)) return fail(QECMC_ERR_INVALID, "alpha noise needs pz_tilde in (0,1] and alpha > 0 (pz_tilde=%g alpha=%g)", p, eta);
        if (code == QECMC_TORIC || code == QECMC_PLANAR) return fail(QECMC_ERR_UNSUPPORTED, "alpha noise is built for the xzzx and rotated codes");
    } else
    if (noise) {
        if (!(p > 0.0) || !(p < 1.0) || !(eta > 0.0)) return fail(QECMC_ERR_INVALID, "biased noise needs p in (0,1) and eta > 0 (p=%g eta=%g)", p, eta);
        if (code == QECMC_TORIC || code == QECMC_PLANAR) return fail(QECMC_ERR_UNSUPPORTED, "biased noise is built for the xzzx and rotated codes (BASELINE config 4)");
    } else if (!(p > 0.0) || !(p <= 0.75)) return fail(QECMC_ERR_INVALID, "p=%g must be in (0, 0.75]", p);
    if (!(p_logical >= 0.0) || !(p_logical <= 1.0)) return fail(QECMC_ERR_INVALID, "p_logical=%g must be in [0,1]", p_logical);
    if (slot >= 0x100u) return fail(QECMC_ERR_INVALID, "slot %u collides with the swap stream id", slot);
    if (int rc = report(rng_range_check("qecmc_chain_update", 0, 1, k0, iters))) return rc;
    ChainArgs a;
    std::memset(&a, 0, sizeof a);
    const double f = noise ? 0.0 : chain_factor(p);
    std::vector<uint32_t> tbl(nq + 1, 0u);
    for (size_t d = 1; d <= nq && !noise; ++d) tbl[d] = thr32(std::pow(f, (double)d));
    for (int d = 1; d <= 4 && !noise; ++d) a.acc44[d] = thr44(std::pow(f, (double)d));
    const std::vector<double> bt = noise == QECMC_NOISE_ALPHA ? alpha_tables(p, eta, nq) : bias_tables(p, noise ? eta : 1.0, nq);
    // one device block, one copy each way: [bias table | acceptance table | states | accepted]
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };     // (every part on a 256-byte boundary, as hipMalloc would place it)
    const size_t o_tbl = up(bt.size() * 8), o_st = o_tbl + up(tbl.size() * 4), o_acc = o_st + up(N * nq), total = o_acc + (accepted_out ? N : 0);
    StagingTrim trim;
    std::vector<uint8_t> &h = staging();
    h.resize(o_acc);
    std::memcpy(h.data(), bt.data(), bt.size() * 8);
    std::memcpy(h.data() + o_tbl, tbl.data(), tbl.size() * 4);
    std::memcpy(h.data() + o_st, states_inout, N * nq);
    DevBuf d;
    HIP_TRY(d.alloc(total));
    HIP_TRY(hipMemcpy(d.p, h.data(), o_acc, hipMemcpyHostToDevice));
    if (accepted_out) a.accepted = d.as<uint8_t>() + o_acc;
    a.states = d.as<uint8_t>() + o_st; a.N = N; a.iters = iters; a.k0 = k0;
    a.thr_logical = p_logical > 0 ? thr64(p_logical) : 0;
    a.acc_tbl = reinterpret_cast<uint32_t *>(d.as<uint8_t>() + o_tbl); a.acc_all = !noise && f >= 1.0;
    a.first_syndrome = first_syndrome; a.slot = slot;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.L = L;
    a.code = code; a.noise = noise; a.bias_tbl = d.as<double>();
    HIP_TRY(launch_chain_update(a, 0));
    if (accepted_out) {
        h.resize(total - o_st);
        HIP_TRY(hipMemcpy(h.data(), d.as<uint8_t>() + o_st, total - o_st, hipMemcpyDeviceToHost));
        std::memcpy(states_inout, h.data(), N * nq);
        std::memcpy(accepted_out, h.data() + (o_acc - o_st), N);
    } else
        HIP_TRY(hipMemcpy(states_inout, d.as<uint8_t>() + o_st, N * nq, hipMemcpyDeviceToHost));
    return 0;
}

int qecmc_chain_update(int code, int L, uint64_t N, uint8_t *states_inout, double p, double p_logical,
                       uint64_t iters, uint64_t seed, uint32_t first_syndrome, uint32_t slot, uint64_t k0)
{
    return chain_update_impl(code, L, N, states_inout, p, 0.0, 0, p_logical, iters, seed, first_syndrome, slot, k0);
}

int qecmc_chain_update_biased(int code, int L, uint64_t N, uint8_t *states_inout, double p, double eta, double p_logical,
                              uint64_t iters, uint64_t seed, uint32_t first_syndrome, uint32_t slot, uint64_t k0)
{
    return chain_update_impl(code, L, N, states_inout, p, eta, 1, p_logical, iters, seed, first_syndrome, slot, k0);
}

int qecmc_chain_update_alpha(int code, int L, uint64_t N, uint8_t *states_inout, double pz_tilde, double alpha, double p_logical,
                             uint64_t iters, uint64_t seed, uint32_t first_syndrome, uint32_t slot, uint64_t k0, uint8_t *accepted_out)
{
    return chain_update_impl(code, L, N, states_inout, pz_tilde, alpha, QECMC_NOISE_ALPHA, p_logical, iters, seed, first_syndrome, slot, k0, accepted_out);
}

// Chain_xyz.update_chain_fast(iters), src/mcmc.py:106-114,162-173, on N independent chains: a stabilizer generator is proposed
// (planar_model._apply_random_stabilizer in the reference, the code's own here) and accepted with probability
// prod_i (p_i / (1 - sum p))^(change of n_i), i = x, y, z.  Draws as the non-top rule of qecmc_chain_update.
int qecmc_chain_update_xyz(int code, int L, uint64_t N, uint8_t *states_inout, const double *p_xyz, uint64_t iters, uint64_t seed,
                           uint32_t first_syndrome, uint32_t slot, uint64_t k0)
{
    PRIM_PROLOGUE();
    if (!states_inout || !p_xyz) return fail(QECMC_ERR_INVALID, "NULL buffer");
    const double tot = (p_xyz[0] + p_xyz[1]) + p_xyz[2];
    if (!(p_xyz[0] > 0) || !(p_xyz[1] > 0) || !(p_xyz[2] > 0) || !(tot < 1.0)) return fail(QECMC_ERR_INVALID, "p_xyz=(%g,%g,%g) must be positive with a sum below 1", p_xyz[0], p_xyz[1], p_xyz[2]);
    if (slot >= 0x100u) return fail(QECMC_ERR_INVALID, "slot %u collides with the swap stream id", slot);
    if (int rc = report(rng_range_check("qecmc_chain_update_xyz", 0, 1, k0, iters))) return rc;
    const std::vector<uint64_t> thr = xyz_thresholds(p_xyz);          // mcmc.py:110,170
    ChainArgs a;
    std::memset(&a, 0, sizeof a);
    DevBuf dthr, dst;
    HIP_TRY(dthr.alloc(729 * 8)); HIP_TRY(dst.alloc(N * nq));
    HIP_TRY(hipMemcpy(dthr.p, thr.data(), 729 * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dst.p, states_inout, N * nq, hipMemcpyHostToDevice));
    a.states = dst.as<uint8_t>(); a.N = N; a.iters = iters; a.k0 = k0; a.first_syndrome = first_syndrome; a.slot = slot;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.L = L; a.code = code; a.noise = 0;
    a.xyz_thr = dthr.as<uint64_t>();
    HIP_TRY(launch_chain_update(a, 0));
    HIP_TRY(hipMemcpy(states_inout, dst.p, N * nq, hipMemcpyDeviceToHost));
    return 0;
}

// The step entry points' plan cache: keyed by the whole parameter block (the fields a plan does not depend on -- seed, first_syndrome,
// steps -- are constant for one ladder anyway), a handful of entries, least recently used out first.  Plans are immutable once
// built (a launch works on a copy of `args`), so concurrent callers may share one.
// (the key: plan_key(), plan_host.hpp)
static int cached_plan(const qecmc_params &pin, std::shared_ptr<const qecmc_plan> *out)
{
    const qecmc_params p = plan_key(pin);
    struct Entry { qecmc_params key; std::shared_ptr<const qecmc_plan> plan; uint64_t used; };
    static std::mutex mu;
    static std::vector<Entry> *cache = new std::vector<Entry>;     // (never destroyed, like the block pool)
    static uint64_t tick = 0;
    constexpr size_t kEntries = 8;
    {
        std::lock_guard<std::mutex> g(mu);
        for (Entry &e : *cache)
            if (std::memcmp(&e.key, &p, sizeof p) == 0) { e.used = ++tick; *out = e.plan; return 0; }
    }
    auto pl = std::make_shared<qecmc_plan>();
    if (int rc = build_plan(&pin, pl.get())) return rc;
    *out = pl;
    std::lock_guard<std::mutex> g(mu);
    if (cache->size() >= kEntries) {
        size_t lru = 0;
        for (size_t i = 1; i < cache->size(); ++i) if ((*cache)[i].used < (*cache)[lru].used) lru = i;
        // (its tables are freed when the last caller still stepping with it returns; every such call ends with a blocking copy)
        (*cache)[lru] = Entry{p, pl, ++tick};
    } else
        cache->push_back(Entry{p, pl, ++tick});
    return 0;
}

static int ladder_step_impl(const qecmc_params *params, uint64_t N, uint8_t *states_inout, uint8_t *flags_inout,
                            uint32_t *tops0_inout, uint16_t *neff_inout, uint64_t iters, uint64_t nsteps, uint64_t step0, uint64_t prop0)
{
    if (!params) return fail(QECMC_ERR_INVALID, "params is NULL");
    qecmc_params p = *params;
    p.iters = iters;
    p.conv_mode = QECMC_CONV_NONE;
    p.replicas = 0;
    if (int rc = report(validate_params(&p))) return rc;
    if (p.scan == QECMC_SCAN_COLOUR) return fail(QECMC_ERR_UNSUPPORTED, "scan = colour starts its ladders from seed configurations (qecmc_pteq_batch / qecmc_pteq_launch_dev)");
    if (!states_inout || !flags_inout || !tops0_inout) return fail(QECMC_ERR_INVALID, "NULL buffer");
    if ((p.noise == QECMC_NOISE_ALPHA) != (neff_inout != nullptr))
        return fail(QECMC_ERR_INVALID, "alpha-noise ladders step through qecmc_ladder_step_alpha (which carries the slots' n_eff), the others through qecmc_ladder_step");
    if (int rc = report(rng_range_check(neff_inout ? "qecmc_ladder_step_alpha" : "qecmc_ladder_step", step0, nsteps, prop0, iters))) return rc;
    if (int rc = use_device(p.device)) return rc;
    if (N == 0) return 0;
    // a Python loop over Ladder.step presents the same parameters every call: the tables of the last few plans are kept
    std::shared_ptr<const qecmc_plan> plan;
    if (int rc = cached_plan(p, &plan)) return rc;
    const qecmc_plan &pl = *plan;
    const size_t nq = pl.args.nq, Nc = pl.args.Nc;
    // one device block, one copy each way: [n_eff records | tops0 | states | flags]
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };     // (every part on a 256-byte boundary, as hipMalloc would place it)
    const size_t o_t0 = neff_inout ? up(N * Nc * 4) : 0, o_st = o_t0 + up(N * 4), o_fl = o_st + up(N * Nc * nq), total = o_fl + N * Nc;
    StagingTrim trim;
    std::vector<uint8_t> &h = staging();
    h.resize(total);
    if (neff_inout) std::memcpy(h.data(), neff_inout, N * Nc * 4);
    std::memcpy(h.data() + o_t0, tops0_inout, N * 4);
    std::memcpy(h.data() + o_st, states_inout, N * Nc * nq);
    std::memcpy(h.data() + o_fl, flags_inout, N * Nc);
    DevBuf d;
    HIP_TRY(d.alloc(total));
    HIP_TRY(hipMemcpy(d.p, h.data(), total, hipMemcpyHostToDevice));
    LadderArgs a = pl.args;
    if (neff_inout) a.neff = d.as<uint32_t>();
    a.states = d.as<uint8_t>() + o_st; a.flags = d.as<uint8_t>() + o_fl; a.tops0 = reinterpret_cast<uint32_t *>(d.as<uint8_t>() + o_t0);
    a.N = N; a.first_syndrome = p.first_syndrome; a.step0 = step0; a.prop0 = prop0; a.nsteps = nsteps;
    a.seed_lo = (uint32_t)p.seed; a.seed_hi = (uint32_t)(p.seed >> 32);      // (the cached tables do not depend on the seed: patched per call)
    a.resume = 1; a.write_states = 1;
    HIP_TRY(launch_ladder(a, 0));
    HIP_TRY(hipMemcpy(h.data(), d.p, total, hipMemcpyDeviceToHost));
    if (neff_inout) std::memcpy(neff_inout, h.data(), N * Nc * 4);
    std::memcpy(tops0_inout, h.data() + o_t0, N * 4);
    std::memcpy(states_inout, h.data() + o_st, N * Nc * nq);
    std::memcpy(flags_inout, h.data() + o_fl, N * Nc);
    return 0;
}

int qecmc_ladder_step(const qecmc_params *params, uint64_t N, uint8_t *states_inout, uint8_t *flags_inout,
                      uint32_t *tops0_inout, uint64_t iters, uint64_t nsteps, uint64_t step0, uint64_t prop0)
{
    return ladder_step_impl(params, N, states_inout, flags_inout, tops0_inout, nullptr, iters, nsteps, step0, prop0);
}

int qecmc_ladder_step_alpha(const qecmc_params *params, uint64_t N, uint8_t *states_inout, uint8_t *flags_inout,
                            uint32_t *tops0_inout, uint16_t *neff_counts_inout, uint64_t iters, uint64_t nsteps,
                            uint64_t step0, uint64_t prop0)
{
    if (!neff_counts_inout) return fail(QECMC_ERR_INVALID, "NULL buffer");
    return ladder_step_impl(params, N, states_inout, flags_inout, tops0_inout, neff_counts_inout, iters, nsteps, step0, prop0);
}

// ---------------------------------------------------------------- PTEQ batch
int qecmc_plan_create(const qecmc_params *params, qecmc_plan **plan_out)
{
    if (!plan_out) return fail(QECMC_ERR_INVALID, "plan_out is NULL");
    *plan_out = nullptr;
    if (int rc = report(validate_params(params))) return rc;
    if (int rc = use_device(params->device)) return rc;
    qecmc_plan *pl = new (std::nothrow) qecmc_plan();
    if (!pl) return fail(QECMC_ERR_INVALID, "out of host memory");
    if (int rc = build_plan(params, pl)) { delete pl; return rc; }
    *plan_out = pl;
    return 0;
}

int qecmc_plan_destroy(qecmc_plan *plan)
{
    // the plan's tables may go back to the block pool and on to another call: wait for the launches that read them (what hipFree used
    // to do) -- on the plan's device, leaving the caller's current device as it was
    if (plan) {
        int cur = -1;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        (void)hipSetDevice(plan->prm.device);
        (void)hipDeviceSynchronize();
        if (have && cur != plan->prm.device) (void)hipSetDevice(cur);
    }
    delete plan;
    return 0;
}

int qecmc_plan_info(const qecmc_plan *plan, uint32_t *lds_bytes, uint32_t *block_threads, uint32_t *syndromes_per_block)
{
    if (!plan) return fail(QECMC_ERR_INVALID, "plan is NULL");
    if (lds_bytes) *lds_bytes = (uint32_t)(plan->d_short_neff ? shortest_lds_bytes(plan->args) : plan->lds_bytes);   // (the shortest-chain kernels' own map)
    if (block_threads) *block_threads = (uint32_t)plan->args.Nc * 64u;
    if (syndromes_per_block) *syndromes_per_block = kSynPerBlock;
    return 0;
}

int qecmc_plan_workspace_bytes(const qecmc_plan *plan, uint64_t N, int with_final_states, uint64_t *bytes_out)
{
    if (!plan || !bytes_out) return fail(QECMC_ERR_INVALID, "NULL argument");
    // what qecmc_pteq_launch_dev(plan, N syndromes, d_final_states given or not) will ask for: a launch that may take the plan's work
    // queue logs one column per lane of the persistent grid, any other one column per ladder
    *bytes_out = plan->workspace(N, plan->takes_queue(with_final_states != 0 || plan->d_swap_acc != nullptr || plan->d_short_neff != nullptr));
    return 0;
}

int qecmc_pteq_launch_dev(qecmc_plan *plan, const void *d_init, uint64_t N, uint32_t first_syndrome, void *d_counts,
                          void *d_samples, void *d_tops0, void *d_steps_done, void *d_converged, void *d_final_states,
                          void *d_workspace, uint64_t workspace_bytes, void *hip_stream)
{
    if (!plan) return fail(QECMC_ERR_INVALID, "plan is NULL");
    if (N == 0) return 0;
    if (!d_init || !d_counts || !d_samples) return fail(QECMC_ERR_INVALID, "NULL device buffer");
    const uint64_t R = plan->args.replicas, M = N * R;              // ladders
    if (M + first_syndrome > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "global ladder index (first_syndrome + N * replicas) exceeds 32 bits");
    if (plan->args.scan == QECMC_SCAN_WAVE && (first_syndrome & 63u))
        return fail(QECMC_ERR_INVALID, "scan = wave: first_syndrome=%u must be a multiple of 64 (a wavefront shares its generator picks)", first_syndrome);
    const bool shortest = plan->d_short_neff != nullptr;      // (qecmc_plan_set_shortest: a lane per ladder for the whole run, never the persistent grid)
    const bool takes_queue = plan->takes_queue(plan->d_swap_acc != nullptr || d_final_states != nullptr || shortest);
    if (shortest) {
        if (plan->d_swap_acc || plan->d_nerr_sum) return fail(QECMC_ERR_UNSUPPORTED, "qecmc_plan_set_shortest: not together with qecmc_plan_set_stats");
        if (int rc = report(shortest_check(plan->prm, kernel_shape(plan->args)))) return rc;
        if (plan->prm.steps == 0 || plan->prm.steps > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "qecmc_plan_set_shortest: steps=%llu must be in [1, 2^32)", (unsigned long long)plan->prm.steps);
        if (plan->args.scan == QECMC_SCAN_WAVE && d_final_states) return fail(QECMC_ERR_UNSUPPORTED, "qecmc_plan_set_shortest: scan = wave writes no final states");
        if (!d_tops0 || !d_steps_done || !d_converged) return fail(QECMC_ERR_INVALID, "NULL device buffer");
        const uint64_t need = shortest_set_need(N, plan->short_cap);
        if (plan->short_set_bytes < need)
            return fail(QECMC_ERR_INVALID, "set workspace of %llu bytes, %llu ladders of capacity %llu take %llu (qecmc_plan_shortest_set_bytes)",
                        (unsigned long long)plan->short_set_bytes, (unsigned long long)N, (unsigned long long)plan->short_cap, (unsigned long long)need);
    }
    {
        const uint64_t need = plan->workspace(N, takes_queue);
        if (need && !d_workspace) return fail(QECMC_ERR_INVALID, "conv_mode error_based needs the workspace of qecmc_plan_workspace_bytes()");
        if (workspace_bytes < need)
            return fail(QECMC_ERR_INVALID, "workspace of %llu bytes, this launch logs %llu (qecmc_plan_workspace_bytes: 2 or 4 bytes per ladder step and column)",
                        (unsigned long long)workspace_bytes, (unsigned long long)need);
    }
    if (R > 1 && (plan->d_swap_acc || plan->d_nerr_sum)) return fail(QECMC_ERR_INVALID, "qecmc_plan_set_stats is per ladder: not with replicas > 1");
    if ((plan->d_swap_acc || plan->d_nerr_sum) && (uint64_t)plan->args.nq * plan->prm.steps > 0xFFFFFFFFull)
        return fail(QECMC_ERR_INVALID, "qecmc_plan_set_stats: nq * steps exceeds the 32-bit error-count sums");
    hipStream_t strm = static_cast<hipStream_t>(hip_stream);
    if (R > 1) {   // the R ladders of a syndrome add into its outputs
        HIP_TRY(hipMemsetAsync(d_counts, 0, N * plan->args.ncls * 4, strm));
        HIP_TRY(hipMemsetAsync(d_samples, 0, N * 4, strm));
        if (d_tops0) HIP_TRY(hipMemsetAsync(d_tops0, 0, N * 4, strm));
        if (d_steps_done) HIP_TRY(hipMemsetAsync(d_steps_done, 0, N * 4, strm));
        if (d_converged) HIP_TRY(hipMemsetAsync(d_converged, 1, N, strm));
    }
    LadderArgs a = plan->args;
    a.swap_acc = plan->d_swap_acc ? plan->d_swap_acc : nullptr;
    a.nerr_sum = plan->d_nerr_sum;
    if (a.nerr_sum && !a.swap_acc) return fail(QECMC_ERR_INVALID, "qecmc_plan_set_stats: d_nerr_sums needs d_swap_accepts");
    a.init = static_cast<const uint8_t *>(d_init);
    a.counts = static_cast<uint32_t *>(d_counts);
    a.samples = static_cast<uint32_t *>(d_samples);
    a.tops0 = static_cast<uint32_t *>(d_tops0);
    a.steps_done = static_cast<uint32_t *>(d_steps_done);
    a.converged = static_cast<uint8_t *>(d_converged);
    a.nlog = static_cast<uint16_t *>(d_workspace);
    a.states = static_cast<uint8_t *>(d_final_states);
    a.write_states = d_final_states != nullptr;
    a.N = M; a.first_syndrome = first_syndrome;
    a.step0 = 0; a.prop0 = 0; a.nsteps = plan->prm.steps; a.resume = 0;
    if (shortest) {
        a.short_neff = plan->d_short_neff; a.short_n = plan->d_short_n; a.short_uniq = plan->d_short_uniq; a.short_over = plan->d_short_over;
        a.short_set = static_cast<unsigned long long *>(plan->d_short_set);
        a.short_slots = (uint32_t)shortest_set_slots(plan->short_cap); a.short_cap = (uint32_t)plan->short_cap;
        HIP_TRY(hipMemsetAsync(plan->d_short_set, 0, shortest_set_need(N, plan->short_cap), strm));
        HIP_TRY(launch_ladder(a, strm));
        return 0;
    }
    if (plan->args.scan == QECMC_SCAN_WAVE && plan->prm.conv_mode != QECMC_CONV_NONE && !takes_queue)
        return fail(QECMC_ERR_UNSUPPORTED, "scan = wave runs the criterion on its persistent grid, where a ladder's lane is reused when it has stopped: no final "
                    "states or per-ladder statistics with conv_mode error_based (and steps must be > 0)");
    if (takes_queue && plan->args.scan == QECMC_SCAN_WAVE) {
        // (the workgroups of the persistent grid own contiguous shares of the batch: no global counter)
        wave_queue_shape(plan->queue_grid, M, &a.grid_cap, &a.wu_chunk);
    } else if (takes_queue) {
        // (one launch at a time per plan: the counter belongs to the plan)
        HIP_TRY(hipMemsetAsync(plan->queue.p, 0, sizeof(uint32_t), strm));
        a.queue = plan->queue.as<uint32_t>();
        a.grid_cap = plan->queue_grid;
    }
    HIP_TRY(launch_ladder(a, strm));
    return 0;
}

int qecmc_plan_set_stats(qecmc_plan *plan, void *d_swap_accepts, void *d_nerr_sums)
{
    if (!plan) return fail(QECMC_ERR_INVALID, "plan is NULL");
    if (d_nerr_sums && !d_swap_accepts) return fail(QECMC_ERR_INVALID, "d_nerr_sums needs d_swap_accepts");
    if (d_swap_accepts && plan->args.Nc < 2) return fail(QECMC_ERR_INVALID, "swap statistics need Nc >= 2");
    if (d_swap_accepts && plan->d_short_neff) return fail(QECMC_ERR_UNSUPPORTED, "qecmc_plan_set_stats: not together with qecmc_plan_set_shortest");
    if (d_swap_accepts && (plan->args.scan == QECMC_SCAN_COLOUR || plan->args.scan == QECMC_SCAN_WAVE)) {
        // the wave and colour layouts count in kernels of their own (choose_wave / choose_colour, kernel_choice.hpp): the chooser says whether one is
        // built for this plan's launches -- fixed-length runs, scan = wave up to 16 state words per rung
        LadderArgs probe = plan->args;
        probe.swap_acc = static_cast<uint32_t *>(d_swap_accepts);
        const KernelKey k = choose_kernel(kernel_shape(probe));
        if (!k.ok()) return fail(QECMC_ERR_UNSUPPORTED, "qecmc_plan_set_stats: %s", k.why);
    } else if (d_swap_accepts && plan->lds_bytes + ladder_stats_lds_bytes(plan->args.Nc) > 160 * 1024)
        return fail(QECMC_ERR_UNSUPPORTED, "no LDS left for the statistics counters at this L / Nc");
    plan->d_swap_acc = static_cast<uint32_t *>(d_swap_accepts);
    plan->d_nerr_sum = static_cast<uint32_t *>(d_nerr_sums);
    return 0;
}

int qecmc_plan_shortest_set_bytes(const qecmc_plan *plan, uint64_t N, uint64_t set_capacity, uint64_t *bytes_out)
{
    if (!plan || !bytes_out) return fail(QECMC_ERR_INVALID, "NULL argument");
    if (set_capacity == 0 || set_capacity > kShortMaxCapacity)
        return fail(QECMC_ERR_INVALID, "set_capacity=%llu must be in [1, 2^26]", (unsigned long long)set_capacity);
    *bytes_out = shortest_set_need(N, set_capacity);
    return 0;
}

int qecmc_plan_set_shortest(qecmc_plan *plan, void *d_short_neff, void *d_short_n, void *d_unique_n, void *d_overflow, void *d_set,
                            uint64_t set_bytes, uint64_t set_capacity)
{
    if (!plan) return fail(QECMC_ERR_INVALID, "plan is NULL");
    if (!d_short_neff && !d_short_n && !d_unique_n && !d_overflow && !d_set) {      // off again
        plan->d_short_neff = nullptr; plan->d_short_n = plan->d_short_uniq = nullptr; plan->d_short_over = nullptr; plan->d_short_set = nullptr;
        plan->short_set_bytes = plan->short_cap = 0;
        return 0;
    }
    if (int rc = report(shortest_check(plan->prm, kernel_shape(plan->args)))) return rc;
    if (plan->d_swap_acc || plan->d_nerr_sum) return fail(QECMC_ERR_UNSUPPORTED, "qecmc_plan_set_shortest: not together with qecmc_plan_set_stats");
    if (!d_short_neff || !d_short_n || !d_unique_n || !d_overflow || !d_set) return fail(QECMC_ERR_INVALID, "NULL device buffer");
    if (set_capacity == 0 || set_capacity > kShortMaxCapacity)
        return fail(QECMC_ERR_INVALID, "set_capacity=%llu must be in [1, 2^26]", (unsigned long long)set_capacity);
    if (shortest_lds_bytes(plan->args) > 160 * 1024)
        return fail(QECMC_ERR_UNSUPPORTED, "qecmc_plan_set_shortest: L=%d Nc=%d needs %zu B of LDS per workgroup (> 160 KiB)", plan->args.L, plan->args.Nc,
                    shortest_lds_bytes(plan->args));
    if (set_bytes < shortest_set_need(1, set_capacity))
        return fail(QECMC_ERR_INVALID, "set workspace of %llu bytes, one ladder of capacity %llu takes %llu (qecmc_plan_shortest_set_bytes)",
                    (unsigned long long)set_bytes, (unsigned long long)set_capacity, (unsigned long long)shortest_set_need(1, set_capacity));
    plan->d_short_neff = static_cast<double *>(d_short_neff); plan->d_short_n = static_cast<uint32_t *>(d_short_n);
    plan->d_short_uniq = static_cast<uint32_t *>(d_unique_n); plan->d_short_over = static_cast<uint8_t *>(d_overflow);
    plan->d_short_set = d_set; plan->short_set_bytes = set_bytes; plan->short_cap = set_capacity;
    return 0;
}

int qecmc_pteq_resume_dev(qecmc_plan *plan, void *d_states, void *d_flags, void *d_tops0, uint64_t N,
                          uint32_t first_syndrome, uint64_t step0, void *d_counts, void *d_samples, void *hip_stream)
{
    if (!plan) return fail(QECMC_ERR_INVALID, "plan is NULL");
    if (N == 0) return 0;
    if (!d_states || !d_flags || !d_tops0) return fail(QECMC_ERR_INVALID, "NULL device buffer");
    if ((d_counts == nullptr) != (d_samples == nullptr)) return fail(QECMC_ERR_INVALID, "d_counts and d_samples go together");
    if (plan->prm.conv_mode != QECMC_CONV_NONE) return fail(QECMC_ERR_INVALID, "qecmc_pteq_resume_dev runs fixed-length chunks: conv_mode must be NONE");
    if (plan->args.replicas > 1) return fail(QECMC_ERR_INVALID, "qecmc_pteq_resume_dev continues single ladders: replicas must be <= 1");
    if (plan->args.noise == QECMC_NOISE_ALPHA) return fail(QECMC_ERR_UNSUPPORTED, "alpha-noise ladders carry n_eff: continue them with qecmc_ladder_step_alpha");
    if (plan->args.scan == QECMC_SCAN_COLOUR) return fail(QECMC_ERR_UNSUPPORTED, "scan = colour starts its ladders from seed configurations: no chunked continuation");
    if (N + first_syndrome > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "global syndrome index exceeds 32 bits");
    if (plan->args.scan == QECMC_SCAN_WAVE && (first_syndrome & 63u))
        return fail(QECMC_ERR_INVALID, "scan = wave: first_syndrome=%u must be a multiple of 64 (a wavefront shares its generator picks)", first_syndrome);
    if (int rc = report(rng_range_check_resume("qecmc_pteq_resume_dev", step0, plan->prm.steps, plan->prm.iters))) return rc;
    LadderArgs a = plan->args;
    a.states = static_cast<uint8_t *>(d_states); a.flags = static_cast<uint8_t *>(d_flags); a.tops0 = static_cast<uint32_t *>(d_tops0);
    a.counts = static_cast<uint32_t *>(d_counts); a.samples = static_cast<uint32_t *>(d_samples);
    a.N = N; a.first_syndrome = first_syndrome;
    a.step0 = step0; a.prop0 = step0 * plan->prm.iters; a.nsteps = plan->prm.steps;
    a.resume = 1; a.write_states = 1; a.accumulate = 1;
    HIP_TRY(launch_ladder(a, static_cast<hipStream_t>(hip_stream)));
    return 0;
}

int qecmc_plan_resume_conv_bytes(const qecmc_plan *plan, uint64_t N, uint64_t log_rows, uint64_t *record_bytes_out, uint64_t *log_bytes_out)
{
    if (!plan || !record_bytes_out || !log_bytes_out) return fail(QECMC_ERR_INVALID, "NULL argument");
    const ResumeConvBytes need = resume_conv_need(plan->prm, N, log_rows);
    *record_bytes_out = need.record;
    *log_bytes_out = need.log;
    return 0;
}

int qecmc_pteq_resume_conv_dev(qecmc_plan *plan, void *d_states, void *d_flags, void *d_tops0, uint64_t N, uint32_t first_syndrome,
                               uint64_t step0, void *d_counts, void *d_samples, void *d_steps_done, void *d_converged, void *d_record,
                               uint64_t record_bytes, void *d_neff, void *d_workspace, uint64_t workspace_bytes, uint64_t log_rows,
                               void *hip_stream)
{
    if (!plan) return fail(QECMC_ERR_INVALID, "plan is NULL");
    if (int rc = report(resume_conv_check(plan->prm))) return rc;
    if (qecmc_device_count() <= 0) return fail(QECMC_ERR_NO_DEVICE, "no HIP device visible: libqecmc has no CPU fallback");
    if (N == 0) return 0;
    if (!d_states || !d_flags || !d_tops0 || !d_counts || !d_samples || !d_steps_done || !d_converged || !d_record || !d_workspace)
        return fail(QECMC_ERR_INVALID, "NULL device buffer");
    const bool alpha = plan->args.noise == QECMC_NOISE_ALPHA;
    if (alpha != (d_neff != nullptr)) return fail(QECMC_ERR_INVALID, "d_neff carries the alpha-noise ladders' n_eff attributes: needed by them, NULL otherwise");
    if (N + first_syndrome > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "global syndrome index exceeds 32 bits");
    const uint64_t steps = plan->prm.steps;
    if (step0 + steps < step0 || step0 + steps > log_rows)
        return fail(QECMC_ERR_INVALID, "step0 + steps = %llu + %llu exceeds the log's %llu rows (row = absolute ladder step: grow the log by appending rows)",
                    (unsigned long long)step0, (unsigned long long)steps, (unsigned long long)log_rows);
    if (step0 + steps > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "step0 + steps exceeds the 32-bit step count of steps_done");
    if (int rc = report(rng_range_check_resume("qecmc_pteq_resume_conv_dev", step0, steps, plan->prm.iters))) return rc;
    const ResumeConvBytes need = resume_conv_need(plan->prm, N, log_rows);
    if (workspace_bytes < need.log)
        return fail(QECMC_ERR_INVALID, "workspace of %llu bytes, a log of %llu rows takes %llu (qecmc_plan_resume_conv_bytes)",
                    (unsigned long long)workspace_bytes, (unsigned long long)log_rows, (unsigned long long)need.log);
    if (record_bytes < need.record)
        return fail(QECMC_ERR_INVALID, "criterion records of %llu bytes, %llu ladders take %llu (qecmc_plan_resume_conv_bytes)",
                    (unsigned long long)record_bytes, (unsigned long long)N, (unsigned long long)need.record);
    LadderArgs a = plan->args;
    a.states = static_cast<uint8_t *>(d_states); a.flags = static_cast<uint8_t *>(d_flags); a.tops0 = static_cast<uint32_t *>(d_tops0);
    a.counts = static_cast<uint32_t *>(d_counts); a.samples = static_cast<uint32_t *>(d_samples);
    a.steps_done = static_cast<uint32_t *>(d_steps_done); a.converged = static_cast<uint8_t *>(d_converged);
    a.crec = static_cast<uint32_t *>(d_record); a.neff = static_cast<uint32_t *>(d_neff);
    a.nlog = static_cast<uint16_t *>(d_workspace);
    a.N = N; a.first_syndrome = first_syndrome;
    a.step0 = step0; a.prop0 = step0 * plan->prm.iters; a.nsteps = steps;
    a.resume = 1; a.write_states = 1; a.accumulate = 1;
    a.queue = nullptr; a.grid_cap = 0;                   // (never the work queue: its lanes run several ladders)
    // (the PRE kernels have no register to spare for the record: a continued launch runs the same kernel without PRE -- the same results)
    a.tune |= QECMC_FLAG_NO_PRE;
    if (const KernelKey k = choose_kernel(kernel_shape(a)); !k.ok() || k.family != kFamLadder || (k.flags & (kPre | kQueue)) || !(k.flags & kConv))
        return fail(QECMC_ERR_UNSUPPORTED, "no criterion kernel that carries its record for this plan%s%s", k.why ? ": " : "", k.why ? k.why : "");
    if (steps == 0) return 0;
    HIP_TRY(launch_ladder(a, static_cast<hipStream_t>(hip_stream)));
    return 0;
}

int qecmc_pteq_batch(const qecmc_params *params, const uint8_t *init, uint64_t N, uint32_t *counts_out,
                     uint32_t *samples_out, uint32_t *tops0_out, uint32_t *steps_done_out, uint8_t *converged_out,
                     uint8_t *final_states_out, qecmc_stats *stats_out)
{
    return qecmc_pteq_batch_stats(params, init, N, counts_out, samples_out, tops0_out, steps_done_out, converged_out,
                                  final_states_out, nullptr, nullptr, stats_out);
}

int qecmc_pteq_batch_stats(const qecmc_params *params, const uint8_t *init, uint64_t N, uint32_t *counts_out,
                           uint32_t *samples_out, uint32_t *tops0_out, uint32_t *steps_done_out, uint8_t *converged_out,
                           uint8_t *final_states_out, uint32_t *swap_accepts_out, uint32_t *nerr_sums_out, qecmc_stats *stats_out)
{
    const auto t0 = std::chrono::steady_clock::now();
    qecmc_plan *pl = nullptr;
    if (int rc = qecmc_plan_create(params, &pl)) return rc;
    struct Guard { qecmc_plan *p; ~Guard() { qecmc_plan_destroy(p); } } guard{pl};   // (synchronises: an error return may leave the launch running)
    if (N == 0) return 0;
    if (!init || !counts_out || !samples_out) return fail(QECMC_ERR_INVALID, "NULL buffer");
    const size_t nq = pl->args.nq, Nc = pl->args.Nc, ncls = pl->args.ncls, R = pl->args.replicas;
    // (the work-queue kernels log one column per lane of the persistent grid, not per ladder: workspace_need knows)
    const uint64_t ws_bytes = pl->workspace(N, pl->takes_queue(swap_accepts_out || nerr_sums_out || final_states_out));
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (ws_bytes > free_b / 2)
        return fail(QECMC_ERR_INVALID, "conv_mode error_based needs %llu bytes of workspace (2*N*steps), %zu free: lower "
                    "`steps` or the batch size", (unsigned long long)ws_bytes, free_b);
    DevBuf di, dc, ds, dt, dsd, dcv, df, dw;
    HIP_TRY(di.alloc(N * nq)); HIP_TRY(dc.alloc(N * ncls * 4)); HIP_TRY(ds.alloc(N * 4)); HIP_TRY(dt.alloc(N * 4));
    HIP_TRY(dsd.alloc(N * 4)); HIP_TRY(dcv.alloc(N));
    if (ws_bytes) HIP_TRY(dw.alloc(ws_bytes));
    if (final_states_out) HIP_TRY(df.alloc(N * R * Nc * nq));
    DevBuf dsa, dns;
    if (swap_accepts_out || nerr_sums_out) {
        HIP_TRY(dsa.alloc(N * (Nc > 1 ? Nc - 1 : 1) * 4));
        if (nerr_sums_out) HIP_TRY(dns.alloc(N * Nc * 4));
        if (int rc = qecmc_plan_set_stats(pl, dsa.p, nerr_sums_out ? dns.p : nullptr)) return rc;
    }
    HIP_TRY(hipMemcpy(di.p, init, N * nq, hipMemcpyHostToDevice));
    EventTimer timer;
    HIP_TRY(timer.start());
    int rc = qecmc_pteq_launch_dev(pl, di.p, N, params->first_syndrome, dc.p, ds.p, dt.p, dsd.p, dcv.p,
                                   final_states_out ? df.p : nullptr, ws_bytes ? dw.p : nullptr, ws_bytes, nullptr);
    if (rc) return rc;
    float ms = 0;
    HIP_TRY(timer.stop(&ms));
    HIP_TRY(hipMemcpy(counts_out, dc.p, N * ncls * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(samples_out, ds.p, N * 4, hipMemcpyDeviceToHost));
    if (tops0_out) HIP_TRY(hipMemcpy(tops0_out, dt.p, N * 4, hipMemcpyDeviceToHost));
    if (steps_done_out) HIP_TRY(hipMemcpy(steps_done_out, dsd.p, N * 4, hipMemcpyDeviceToHost));
    if (converged_out) HIP_TRY(hipMemcpy(converged_out, dcv.p, N, hipMemcpyDeviceToHost));
    if (final_states_out) HIP_TRY(hipMemcpy(final_states_out, df.p, N * R * Nc * nq, hipMemcpyDeviceToHost));
    if (swap_accepts_out) HIP_TRY(hipMemcpy(swap_accepts_out, dsa.p, N * (Nc - 1) * 4, hipMemcpyDeviceToHost));
    if (nerr_sums_out) HIP_TRY(hipMemcpy(nerr_sums_out, dns.p, N * Nc * 4, hipMemcpyDeviceToHost));
    if (stats_out) {
        stats_out->proposals = N * R * Nc * params->iters * params->steps;   // upper bound when the criterion stops early
        stats_out->swap_tests = N * R * (Nc - 1) * params->steps;
        stats_out->kernel_ms = ms;
        stats_out->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

int qecmc_pteq_batch_shortest(const qecmc_params *params, const uint8_t *init, uint64_t N, uint64_t set_capacity, uint32_t *counts_out,
                              uint32_t *samples_out, uint32_t *tops0_out, uint32_t *steps_done_out, uint8_t *converged_out, double *short_neff_out,
                              uint32_t *short_n_out, uint32_t *unique_n_out, uint8_t *overflow_out, qecmc_stats *stats_out)
{
    const auto t0 = std::chrono::steady_clock::now();
    // everything the host alone can refuse comes before the device is looked for
    if (int rc = report(validate_params(params))) return rc;
    {
        HostPlan hp;
        if (int rc = report(plan_host(*params, hp))) return rc;
        if (int rc = report(shortest_check(*params, hp.shape))) return rc;
    }
    if (set_capacity == 0 || set_capacity > kShortMaxCapacity)
        return fail(QECMC_ERR_INVALID, "set_capacity=%llu must be in [1, 2^26]", (unsigned long long)set_capacity);
    if (params->steps == 0 || params->steps > 0xFFFFFFFFull)
        return fail(QECMC_ERR_INVALID, "qecmc_plan_set_shortest: steps=%llu must be in [1, 2^32)", (unsigned long long)params->steps);
    if (N != 0 && (!init || !counts_out || !samples_out || !short_neff_out || !short_n_out || !unique_n_out || !overflow_out))
        return fail(QECMC_ERR_INVALID, "NULL buffer");
    qecmc_plan *pl = nullptr;
    if (int rc = qecmc_plan_create(params, &pl)) return rc;
    struct Guard { qecmc_plan *p; ~Guard() { qecmc_plan_destroy(p); } } guard{pl};   // (synchronises: an error return may leave the launch running)
    if (N == 0) return 0;
    const size_t nq = pl->args.nq, ncls = pl->args.ncls;
    const uint64_t ws_bytes = pl->workspace(N, false), set_bytes = shortest_set_need(N, set_capacity);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (ws_bytes + set_bytes > free_b / 2)
        return fail(QECMC_ERR_INVALID, "the criterion's log and the ladders' sets need %llu + %llu bytes, %zu free: lower `steps`, set_capacity or the batch size",
                    (unsigned long long)ws_bytes, (unsigned long long)set_bytes, free_b);
    DevBuf di, dc, ds, dt, dsd, dcv, dw, dne, dsn, dun, dov, dset;
    HIP_TRY(di.alloc(N * nq)); HIP_TRY(dc.alloc(N * ncls * 4)); HIP_TRY(ds.alloc(N * 4)); HIP_TRY(dt.alloc(N * 4));
    HIP_TRY(dsd.alloc(N * 4)); HIP_TRY(dcv.alloc(N));
    HIP_TRY(dne.alloc(N * 4 * 8)); HIP_TRY(dsn.alloc(N * 4 * 4)); HIP_TRY(dun.alloc(N * 4 * 4)); HIP_TRY(dov.alloc(N)); HIP_TRY(dset.alloc(set_bytes));
    if (ws_bytes) HIP_TRY(dw.alloc(ws_bytes));
    if (int rc = qecmc_plan_set_shortest(pl, dne.p, dsn.p, dun.p, dov.p, dset.p, set_bytes, set_capacity)) return rc;
    HIP_TRY(hipMemcpy(di.p, init, N * nq, hipMemcpyHostToDevice));
    EventTimer timer;
    HIP_TRY(timer.start());
    if (int rc = qecmc_pteq_launch_dev(pl, di.p, N, params->first_syndrome, dc.p, ds.p, dt.p, dsd.p, dcv.p, nullptr, ws_bytes ? dw.p : nullptr, ws_bytes, nullptr))
        return rc;
    float ms = 0;
    HIP_TRY(timer.stop(&ms));
    HIP_TRY(hipMemcpy(counts_out, dc.p, N * ncls * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(samples_out, ds.p, N * 4, hipMemcpyDeviceToHost));
    if (tops0_out) HIP_TRY(hipMemcpy(tops0_out, dt.p, N * 4, hipMemcpyDeviceToHost));
    if (steps_done_out) HIP_TRY(hipMemcpy(steps_done_out, dsd.p, N * 4, hipMemcpyDeviceToHost));
    if (converged_out) HIP_TRY(hipMemcpy(converged_out, dcv.p, N, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(short_neff_out, dne.p, N * 4 * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(short_n_out, dsn.p, N * 4 * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(unique_n_out, dun.p, N * 4 * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(overflow_out, dov.p, N, hipMemcpyDeviceToHost));
    if (stats_out) {
        const size_t Nc = pl->args.Nc;
        stats_out->proposals = N * Nc * params->iters * params->steps;   // upper bound when the criterion stops early
        stats_out->swap_tests = N * (Nc - 1) * params->steps;
        stats_out->kernel_ms = ms;
        stats_out->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

int qecmc_ptdc_batch(const qecmc_params *params, const uint8_t *init, uint64_t N, int32_t droplets, uint32_t flags,
                     uint32_t *hist_out, uint32_t *m_out, qecmc_stats *stats_out)
{
    return qecmc_ptdc_batch_conv(params, init, N, droplets, flags, 0.0, hist_out, m_out, nullptr, stats_out);
}

int qecmc_ptdc_batch_conv(const qecmc_params *params, const uint8_t *init, uint64_t N, int32_t droplets, uint32_t flags,
                          double conv_mult, uint32_t *hist_out, uint32_t *m_out, uint32_t *steps_done_out, qecmc_stats *stats_out)
{
    return qecmc_ptdc_batch_xyz(params, init, N, droplets, flags, conv_mult, nullptr, hist_out, m_out, steps_done_out, nullptr, nullptr, stats_out);
}

int qecmc_ptdc_batch_xyz(const qecmc_params *params, const uint8_t *init, uint64_t N, int32_t droplets, uint32_t flags,
                         double conv_mult, const double *p_xyz_sampling, uint32_t *hist_out, uint32_t *m_out,
                         uint32_t *steps_done_out, uint32_t *xyz_out, uint32_t *xyz_count_out, qecmc_stats *stats_out)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!params) return fail(QECMC_ERR_INVALID, "params is NULL");
    if (!(conv_mult >= 0.0) || !std::isfinite(conv_mult)) return fail(QECMC_ERR_INVALID, "conv_mult=%g must be finite and >= 0", conv_mult);
    qecmc_params p = *params;
    p.p_logical = 0.0;                                   // Ladder(p_sampling, code, Nc): decoders.py:182,196
    p.conv_mode = QECMC_CONV_NONE;
    p.replicas = 0;                                      // (droplets are this entry point's own replica dimension)
    std::vector<uint64_t> xyz_thr;
    if (p_xyz_sampling) {
        // Chain_xyz (mcmc.py:106-114): factors = p_xyz / (1 - p_xyz.sum()), accept iff u < (factors ** change).prod() (:170)
        const double *q = p_xyz_sampling;
        const double tot = (q[0] + q[1]) + q[2];
        if (!(q[0] > 0) || !(q[1] > 0) || !(q[2] > 0) || !(tot < 1.0)) return fail(QECMC_ERR_INVALID, "p_xyz_sampling=(%g,%g,%g) must be positive with a sum below 1", q[0], q[1], q[2]);
        if (p.Nc != 1) return fail(QECMC_ERR_INVALID, "Chain_xyz is a single chain (mcmc.py:106): Nc=%d must be 1", p.Nc);
        if (p.code == QECMC_TORIC) return fail(QECMC_ERR_UNSUPPORTED, "Chain_xyz is built for the planar, xzzx and rotated codes (the reference's runs the planar stencil, mcmc.py:164)");
        xyz_thr = xyz_thresholds(q);
        p.p = tot <= 0.75 ? tot : 0.75;                                           // unused by the rule; keeps the plan's tables valid
    }
    if (p.noise == QECMC_NOISE_ALPHA) {
        // STDC_droplet_alpha (decoders.py:510-534): Chain_alpha single chains, `update_chain(5)` per step
        if (p.Nc != 1) return fail(QECMC_ERR_UNSUPPORTED, "the unique-chain estimators run Chain_alpha as single chains (decoders.py:510): Nc=%d must be 1", p.Nc);
        if (p_xyz_sampling) return fail(QECMC_ERR_INVALID, "p_xyz_sampling and alpha noise exclude each other");
    } else
    if (p.noise != QECMC_NOISE_DEPOLARIZING) return fail(QECMC_ERR_UNSUPPORTED, "PTDC is defined for the depolarizing ladder (decoders.py:168)");
    if (p.scan != QECMC_SCAN_RANDOM) return fail(QECMC_ERR_UNSUPPORTED, "PTDC runs the reference's random-scan ladder");
    if (droplets < 1) return fail(QECMC_ERR_INVALID, "droplets=%d must be >= 1", droplets);
    if (flags & ~3u) return fail(QECMC_ERR_INVALID, "unknown flags 0x%x", flags);
    const bool init_per_droplet = flags & QECMC_PTDC_INIT_PER_DROPLET, per_rung = flags & QECMC_PTDC_SET_PER_RUNG;
    qecmc_plan *pl = nullptr;
    if (int rc = qecmc_plan_create(&p, &pl)) return rc;
    struct Guard { qecmc_plan *p; ~Guard() { qecmc_plan_destroy(p); } } guard{pl};   // (synchronises: an error return may leave the launch running)
    if (N == 0) return 0;
    if (!init || !hist_out) return fail(QECMC_ERR_INVALID, "NULL buffer");
    const size_t nq = pl->args.nq, Nc = pl->args.Nc, ncls = pl->args.ncls, D = (size_t)droplets;
    const uint64_t M = N * ncls * D;                                  // ladders
    const uint64_t sets = per_rung ? M * Nc : N * ncls;               // PTRC: one per (ladder, rung); PTDC: one per (syndrome, class)
    if (M + p.first_syndrome > 0xFFFFFFFFull) return fail(QECMC_ERR_INVALID, "first_syndrome + N * classes * droplets = %llu ladders exceed the 32-bit syndrome index", (unsigned long long)(M + p.first_syndrome));
    uint64_t cap = 16;
    while (cap < 2 * p.steps * (per_rung ? 1 : Nc * D)) cap <<= 1;    // twice the insertions one set can see
    if (per_rung) conv_mult = 0.0;                                    // PTRC_droplet's stop is commented out (decoders.py:627-630)
    const bool own = conv_mult != 0.0 && D > 1;                       // the stop looks at each droplet's own dictionary
    uint64_t own_cap = 16;
    while (own_cap < 2 * p.steps * Nc) own_cap <<= 1;
    const uint64_t maxu = p.steps * Nc * D;                           // distinct chains a (syndrome, class) set can hold
    if (xyz_out && per_rung) return fail(QECMC_ERR_INVALID, "xyz_out is defined for the per-class sets, not with QECMC_PTDC_SET_PER_RUNG");
    if (xyz_out && nq > 1023) return fail(QECMC_ERR_UNSUPPORTED, "xyz_out packs counts in 10 bits: nq=%zu", nq);
    const uint64_t need = sets * cap * 8 + M * nq + sets * (nq + 1) * 8 + (own ? M * own_cap * 8 : 0) + M * 4 + (xyz_out ? sets * (maxu + 1) * 4 : 0);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b - free_b / 8)
        return fail(QECMC_ERR_INVALID, "PTDC needs %llu bytes of device memory (%llu sets x %llu keys), %zu free: lower N, droplets or steps",
                    (unsigned long long)need, (unsigned long long)sets, (unsigned long long)cap, free_b);
    // one start per ladder; the kernel copies it into every rung and sets the top flag (Ladder.__init__, mcmc.py:72-75)
    std::vector<uint8_t> st((size_t)M * nq);
    for (uint64_t sc = 0; sc < N * ncls; ++sc)
        for (size_t d = 0; d < D; ++d)
            std::memcpy(&st[(sc * D + d) * nq], init + (init_per_droplet ? sc * D + d : sc) * nq, nq);
    DevBuf ds, dtab, dh, dm, down, dsd, dxyz, dxc, dthr;
    HIP_TRY(ds.alloc(st.size()));
    if (xyz_out) {
        HIP_TRY(dxyz.alloc(sets * maxu * 4)); HIP_TRY(hipMemset(dxyz.p, 0xFF, sets * maxu * 4));
        HIP_TRY(dxc.alloc(sets * 4)); HIP_TRY(hipMemset(dxc.p, 0, sets * 4));
    }
    if (!xyz_thr.empty()) { HIP_TRY(dthr.alloc(729 * 8)); HIP_TRY(hipMemcpy(dthr.p, xyz_thr.data(), 729 * 8, hipMemcpyHostToDevice)); }
    if (own) { HIP_TRY(down.alloc(M * own_cap * 8)); HIP_TRY(hipMemset(down.p, 0, M * own_cap * 8)); }
    if (steps_done_out) HIP_TRY(dsd.alloc(M * 4));
    HIP_TRY(dtab.alloc(sets * cap * 8)); HIP_TRY(dh.alloc(sets * (nq + 1) * 4));
    if (m_out) { HIP_TRY(dm.alloc(sets * (nq + 1) * 4)); HIP_TRY(hipMemset(dm.p, 0, sets * (nq + 1) * 4)); }
    HIP_TRY(hipMemcpy(ds.p, st.data(), st.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dtab.p, 0, sets * cap * 8)); HIP_TRY(hipMemset(dh.p, 0, sets * (nq + 1) * 4));
    EventTimer timer;
    HIP_TRY(timer.start());
    // ONE launch: the ladder kernel inserts every rung's configuration into its set after every step (USET instantiation)
    LadderArgs a = pl->args;
    a.init = ds.as<uint8_t>();
    a.N = M; a.first_syndrome = p.first_syndrome; a.nsteps = p.steps; a.step0 = 0; a.prop0 = 0; a.resume = 0; a.write_states = 0;
    a.uset_tab = reinterpret_cast<unsigned long long *>(dtab.p); a.uset_cap = cap; a.uset_hist = dh.as<uint32_t>();
    a.uset_mhist = m_out ? dm.as<uint32_t>() : nullptr; a.uset_D = (uint32_t)D; a.uset_per_rung = per_rung ? 1 : 0;
    a.uset_conv_mult = conv_mult; a.uset_own = own ? reinterpret_cast<unsigned long long *>(down.p) : nullptr; a.uset_own_cap = own_cap;
    a.steps_done = steps_done_out ? dsd.as<uint32_t>() : nullptr;
    a.uset_xyz = xyz_out ? dxyz.as<uint32_t>() : nullptr; a.uset_xyz_cnt = xyz_out ? dxc.as<uint32_t>() : nullptr; a.uset_xyz_stride = maxu;
    a.xyz_thr = xyz_thr.empty() ? nullptr : dthr.as<uint64_t>();
    {
        const hipError_t e = launch_ladder(a, 0);
        if (e != hipSuccess) return fail(QECMC_ERR_HIP, "PTDC launch: %s", hipGetErrorString(e));
    }
    float ms = 0;
    HIP_TRY(timer.stop(&ms));
    HIP_TRY(hipMemcpy(hist_out, dh.p, sets * (nq + 1) * 4, hipMemcpyDeviceToHost));
    if (m_out) HIP_TRY(hipMemcpy(m_out, dm.p, sets * (nq + 1) * 4, hipMemcpyDeviceToHost));
    if (steps_done_out) HIP_TRY(hipMemcpy(steps_done_out, dsd.p, M * 4, hipMemcpyDeviceToHost));
    if (xyz_out) HIP_TRY(hipMemcpy(xyz_out, dxyz.p, sets * maxu * 4, hipMemcpyDeviceToHost));
    if (xyz_out && xyz_count_out) HIP_TRY(hipMemcpy(xyz_count_out, dxc.p, sets * 4, hipMemcpyDeviceToHost));
    if (stats_out) {
        stats_out->proposals = M * Nc * p.iters * p.steps;
        stats_out->swap_tests = M * (Nc - 1) * p.steps;
        stats_out->kernel_ms = ms;
        stats_out->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

}  // extern "C"
