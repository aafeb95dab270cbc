// The body of the scan = 3 kernels (ladder_wu.hpp), included as text into ladder_wu_kernel and into ladder_wu_stats_kernel: the two are one program
// under two names, told apart by the compile-time STATS alone (wrapped in a force-inlined function the body compiles to other code in the
// kernels that sit at their register budget, DESIGN.md 7).  The includer provides CODE, WV, CONV, QUEUE, IT, ALPHA, STATS, SHORT, LONG and the argument `a`.
    typedef typename WuVec<WV>::type vec_t;
    extern __shared__ uint32_t lds[];
    const int NC = a.Nc, W = a.W, L = a.L, nq = a.nq, ncls = a.ncls;
    const int nthreads = NC * 64;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);      // this wave's rung (fixed: states move)
    const WuLds o = wu_lds(NC, W, ncls, L, CONV, ALPHA, SHORT, wu_frame_steps(WV, CONV, ALPHA, IT));
    uint32_t *xbuf = lds + o.xbuf, *rec = lds + o.rec, *hist = lds + o.hist, *thrT = lds + o.thr;
    uint32_t *swapT = lds + o.swapT, *lml = lds + o.lml;
    volatile uint32_t *stopf = lds + o.stop;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(wu_lds_ptr)lds;                    // LDS byte address of the dynamic segment
    const uint32_t R = a.replicas;
    // the workgroup's share of the batch: 64 ladders, or -- QUEUE -- a.wu_chunk of them, taken 64 at a time
    const uint64_t s0 = (uint64_t)blockIdx.x * (QUEUE ? (uint64_t)a.wu_chunk : 64u);
    const uint64_t s1 = QUEUE ? (s0 + a.wu_chunk < a.N ? s0 + a.wu_chunk : a.N) : a.N;
    const int cnt = s1 > s0 ? (int)((s1 - s0) < 64u ? (s1 - s0) : 64u) : 0;
    const bool live = lane < cnt;
    const bool top = slot == (uint32_t)(NC - 1);                                  // (the launcher guarantees that this rung accepts every move)

    // ---- tables
    for (int i = tid; i < ncls * 64; i += nthreads) hist[i] = 0;
    if (tid < 4) stopf[tid] = tid == 2 ? (uint32_t)s0 + 64u : 0u;   // [0], [1]: stop, by step parity; [2]: the workgroup's queue (next unassigned ladder)
    if constexpr (CONV) {
        uint32_t *bk = lds + o.bk, *mail = lds + o.mail;
        for (int i = tid; i < (ALPHA ? kWuBkAlpha : kWuBk) * 64; i += nthreads) {
            const int row = i >> 6, l = i & 63;
            bk[i] = row == 9 ? (l < cnt ? 8u : 0u) : row == 12 ? (uint32_t)s0 + (uint32_t)l : 0u;                   // state: has; the lane's ladder
        }
        for (int i = tid; i < 128; i += nthreads) mail[i] = kWuKeep;
    }
    if constexpr (SHORT) {
        for (int i = tid; i < kShortRows * 64; i += nthreads) lds[o.sst + i] = short_init_word(i >> 6);
    }
    if constexpr (ALPHA) {
        // (D_xy, D_z) of a proposal as two fp16 integers, at byte offset 4 ((D_z + 4) + 9 (D_xy + 4)); ln(pz_i / pz_i+1) of the rung pairs
        for (int i = tid; i < 81; i += nthreads) {
            const wu_half2 h = {(_Float16)(float)(i / 9 - 4), (_Float16)(float)(i % 9 - 4)};
            lds[o.cht + i] = __builtin_bit_cast(uint32_t, h);
        }
        for (int i = tid; i < NC - 1; i += nthreads) reinterpret_cast<double *>(lds + o.lnb)[i] = a.alpha_lnb[i];
    }
    for (int i = tid; i < NC * 18 && !ALPHA; i += nthreads) {
        const int c = i / 18, r = i - c * 18, hi = r < 9, idx = hi ? r : r - 9;
        // dE <= 0 (idx <= 4): always accepted -- a high part no 12-bit uniform reaches; dE = 1..4: ceil(f^dE 2^44)
        const uint64_t t44 = idx <= 4 ? (1ull << 44) : a.acc_thr44[c][idx - 5];
        thrT[i] = hi ? (uint32_t)(t44 >> 32) : (uint32_t)t44;
    }
    for (int i = tid; i < (NC - 1) * kSwapFast && !ALPHA; i += nthreads) {
        const int pr = i / kSwapFast, d = i - pr * kSwapFast;
        swapT[i] = (d >= 1 && d <= nq) ? (uint32_t)a.swap_thr[(size_t)pr * (nq + 1) + d] : 0u;
    }
    for (int i = tid; i < 4 * (L + 1) * WV + 64; i += nthreads) {          // rows padded to WV words
        const int row = i / WV, w = i - row * WV;
        lml[i] = (row < 4 * (L + 1) && w < W) ? a.lmask[row * W + w] : 0u;
    }

    // ---- stage this rung's state into registers: Ladder.__init__ copies the seed into every rung (mcmc.py:72), or resume
    vec_t st;
    wu_def<WV>(st);
    uint32_t n4 = 0, cls = 0, flag = top ? 1u : 0u;
    const uint64_t ladder = s0 + (uint64_t)(live ? lane : 0);
#define QECMC_WU_ZERO(w) if constexpr (w < WV) wu_set<WV, w>(st, 0u);
    WU_EACH(QECMC_WU_ZERO)
#undef QECMC_WU_ZERO
    if (cnt > 0) {
        const int rows = wu_rows(W, CONV);                            // rows of a rung's region of the exchange buffer
        const wu_lds_rw xcol = (wu_lds_rw)(uintptr_t)lds0 + (slot * (uint32_t)rows) * 64u + (uint32_t)lane;
        wu_stage_lds<CODE>(a, ladder, slot, xcol, n4, cls, 0, WV == 32 ? kWuHalf : W, rows);
        const uint32_t xme = lds0 + (uint32_t)lane * 4u + slot * (uint32_t)(rows * 256);
        const int Wl = W;
#define QECMC_WU_MINE(w) if constexpr (w < WV && w < kWuHalf) { if (WV == 32 || !CONV || w < wu_words_min(WV) || w < Wl) wu_ds_read<WV, w>(st, xme); }
        WU_EACH(QECMC_WU_MINE)
#undef QECMC_WU_MINE
        wu_ds_wait<WV>(st);
        if constexpr (WV == 32) {
            // (the upper half through the same rows: this lane's own column, which nobody else reads)
            wu_stage_lds<CODE>(a, ladder, slot, xcol, n4, cls, kWuHalf, W, rows);
#define QECMC_WU_MINE_HI(w) if constexpr (w < WV && w >= kWuHalf) wu_ds_read<WV, w, w - kWuHalf>(st, xme);
            WU_EACH(QECMC_WU_MINE_HI)
#undef QECMC_WU_MINE_HI
            wu_ds_wait<WV>(st);
        }
        if (a.resume) flag = a.flags[ladder * NC + slot];
    }
    // the booking wave's per-ladder bookkeeping (the criterion kernels: in LDS): wave 0's, or -- the walked forms of the lean tail, ladder_wu.hpp
    // kWuTopBooks -- the top rung's, which hands tops0 and samples to wave 0's write-out below
    const bool tbooks = wu_top_books_family(WV, CONV, ALPHA, STATS, LONG) && a.wu_once != 0;
    uint32_t tops0 = 0;
    if ((tbooks ? top : slot == 0) && a.resume && live) tops0 = a.tops0[s0 + lane];
    __syncthreads();

    uint32_t nef0 = 0;
    if constexpr (ALPHA) { const uint32_t c3 = wu_counts_packed<WV>(st, 0x55555555u); nef0 = ((c3 >> 10) & 1023u) | ((c3 >> 20) << 16); }   // Chain_alpha.__init__, mcmc_alpha.py:18-22
    WuCtx cx{n4, cls, flag, tops0, 0u, 0u, 0u, 0u, nef0};
    WuEnv ev;
    ev.lds0 = lds0; ev.thr_off = (uint32_t)((o.thr + (int)slot * 18) * 4); ev.lml_off = (uint32_t)(o.lml * 4); ev.cht_off = (uint32_t)(o.cht * 4); ev.frm_off = (uint32_t)(o.frm * 4); ev.slot = slot;
    ev.grp = (a.first_syndrome >> 6) + (uint32_t)blockIdx.x;         // the wavefront's shared picks: its position in the grid
    ev.lad = live ? (uint32_t)ladder : kWuDead;
    ev.lane = lane; ev.chunk_hi = s1;
    // (the two roles are separate loops: they meet at the step's barriers)
    if constexpr (wu_frame_steps(WV, CONV, ALPHA, IT) != 0) wu_pin<WV>(st);
    if (top) wu_run<CODE, WV, CONV, QUEUE, true, IT, ALPHA, STATS, SHORT, LONG>(a, st, cx, ev);
    else wu_run<CODE, WV, CONV, QUEUE, false, IT, ALPHA, STATS, SHORT, LONG>(a, st, cx, ev);
    if constexpr (wu_frame_steps(WV, CONV, ALPHA, IT) != 0) wu_pin<WV>(st);
    if constexpr (QUEUE) return;                                      // (every ladder wrote its results when it ended)
    if constexpr (STATS) {
        // qecmc_plan_set_stats: this wave's two counters of the lane's ladder -- pair slot - 1 (mcmc.py:97-99) and the slot's summed error counts
        if (live) {
            if (slot != 0) a.swap_acc[ladder * (uint64_t)(NC - 1) + (slot - 1u)] = cx.swapc;
            if (a.nerr_sum != nullptr) a.nerr_sum[ladder * (uint64_t)NC + slot] = cx.nsum;
        }
    }
    n4 = cx.n4; cls = cx.cls; flag = cx.flag; tops0 = cx.tops0;
    uint32_t samples = cx.samples, done = 0, conv_ok = 0, steps_done = 0;
    const uint32_t xaddr = lds0 + (uint32_t)lane * 4u;
    // ---- results
    __syncthreads();
    if constexpr (CONV) {
        const uint32_t *bk = lds + o.bk + lane;
        tops0 = bk[0]; samples = bk[64]; done = bk[576] & 1u; steps_done = bk[640]; conv_ok = bk[704];
    }
    const int rows = wu_rows(W, CONV);
    {
        const int Wl = W;
        const uint32_t xo = xaddr + slot * (uint32_t)(rows * 256);
        WU_EACH(QECMC_WU_PUT)
        wu_ds_wait<WV>(st);
        rec[slot * 64u + (uint32_t)lane] = pack_info(n4 >> 2, slot, cls, flag);
        // (rows 0 and 1 of swd -- a walked ladder has five rungs or more -- are dead behind the barrier above: the last conversion of a swap word in place,
        // by a wave that had left the step loop, lies in front of it)
        if (tbooks && top) { lds[o.swd + lane] = tops0; lds[o.swd + 64 + lane] = samples; }
    }
    __syncthreads();
    if (tbooks && slot == 0) { tops0 = lds[o.swd + lane]; samples = lds[o.swd + 64 + lane]; }
    if (a.counts != nullptr)
#pragma unroll 1
        for (int i = tid; i < cnt * ncls; i += nthreads) {
            const int j = i / ncls, c = i - j * ncls;
            const uint32_t v = hist[c * 64 + j];
            if (R > 1) { if (v) atomicAdd(a.counts + ((s0 + (uint64_t)j) / R) * ncls + c, v); }
            else if (a.accumulate) a.counts[s0 * ncls + i] += v;
            else a.counts[s0 * ncls + i] = v;
        }
    if (slot == 0 && live) {
        store_ladder_results(a.samples, a.tops0, a.steps_done, a.converged, R > 1 ? (s0 + lane) / R : s0 + lane, R, a.accumulate != 0, samples, tops0,
                             done ? steps_done : (uint32_t)a.nsteps, conv_ok != 0);
        if (R <= 1 && a.flags != nullptr)
            for (int c = 0; c < NC; ++c) a.flags[(s0 + lane) * NC + c] = (uint8_t)info_flag(rec[c * 64 + lane]);
    }
    if (a.write_states && a.states != nullptr) {
        // (the words the exchange buffer holds: all of them, or -- 32-word kernels -- the lower half, then the upper one)
        uint8_t *dst = a.states + s0 * (uint64_t)NC * nq;
        const int per = NC * nq, total = cnt * per;
        auto copy = [&](int w_lo, int w_hi) {
#pragma unroll 1
            for (int i = tid; i < total; i += nthreads) {
                const int j = i / per, rem = i - j * per, c = rem / nq, q = rem - c * nq;
                const int pos = CODE == kCodeToric ? (q >= L * L ? 2 * (q - L * L) + 1 : 2 * q) : q, w = pos >> 4;   // (the wave layout, tables.hpp wave_position)
                if (w >= w_lo && w < w_hi) dst[i] = (uint8_t)((xbuf[(c * rows + (w - w_lo)) * 64 + j] >> ((pos & 15) * 2)) & 3u);
            }
        };
        copy(0, rows);
        if constexpr (WV == 32) {
            const int Wl = W;
            const uint32_t xo = xaddr + slot * (uint32_t)(rows * 256);
            __syncthreads();
            WU_EACH(QECMC_WU_PUT_HI)
            wu_ds_wait<WV>(st);
            __syncthreads();
            copy(kWuHalf, W);
        }
    }
