"""Criterion-stopped PTEQ runs continued from device state (qecmc_pteq_resume_conv_dev, harness.LadderRun(conv_criteria=...)): a run cut into
chunks is the one long run bit for bit -- every stop decision and the step it is taken at -- against the CPU oracle and against one
pteq_batch launch of the total length.  The parameters of every case were chosen on the CPU with the oracle so that the carry is exercised: a
ladder converges inside the first chunk, one converges in a later chunk, and one is still running at the horizon (asserted below on the oracle's
own result)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return qecmc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _init(name, N, L, p, seed):
    rng = np.random.default_rng(seed)
    shape = (N, 2, L, L) if name == "toric" else (N, L, L)
    return (rng.integers(1, 4, size=shape) * (rng.random(shape) < p)).astype(np.uint8)


# name, L, Nc, N, p, tops_burn, criterion, rule (eta / alpha / scan), chunks.  first_syndrome = 7 everywhere; N = 70, 77: ragged last groups
CRIT = dict(TOPS=3, SEQ=1, eps=0.3)
CASES = {
    "toric5": ("toric", 5, 5, 80, 0.12, 2, CRIT, {}, (1300, 1, 900, 799)),
    "toric9": ("toric", 9, 8, 70, 0.3, 0, dict(TOPS=1, SEQ=0, eps=0.5), {}, (1500, 1, 700, 799)),
    "xzzx5": ("xzzx", 5, 5, 80, 0.12, 2, CRIT, {}, (200, 1, 99, 100)),
    "biased": ("xzzx", 5, 5, 80, 0.12, 2, CRIT, dict(eta=3.0), (50, 1, 149, 200)),
    "alpha": ("rotated", 5, 5, 80, 0.12, 2, CRIT, dict(alpha=1.5), (400, 1, 400, 399)),
    "sweep": ("toric", 5, 5, 77, 0.12, 2, CRIT, dict(scan="sweep"), (600, 1, 500, 399)),
}
OUT = ("counts", "samples", "tops0", "steps_done", "converged")


def _setup(q, orc, case):
    name, L, Nc, N, p, tops_burn, crit, rule, chunks = CASES[case]
    init = _init(name, N, L, 0.1, 11)
    H = sum(chunks)
    okw = dict(rule)
    if "eta" in okw:
        okw["noise"] = orc.BIASED
    if "alpha" in okw:
        okw["noise"] = orc.ALPHA
    if okw.get("scan") == "sweep":
        okw["scan"] = 1
    ref = orc.pteq_batch(getattr(orc, name.upper()), init, p, Nc, H, iters=10, tops_burn=tops_burn, seed=21, first_syndrome=7,
                         conv_criteria="error_based", return_states=True, **crit, **okw)
    ref = {k: (v.astype(np.uint32) if k in ("samples", "tops0", "steps_done") else v) for k, v in ref.items()}
    kw = dict(Nc=Nc, iters=10, tops_burn=tops_burn, seed=21, first_syndrome=7, code=getattr(q, name.upper()), conv_criteria="error_based", **crit, **rule)
    return init, p, H, chunks, ref, kw


def _assert_same(got, ref, what):
    for k in OUT:
        assert np.array_equal(got[k], ref[k]), (what, k)
    live = ~ref["converged"]
    assert np.array_equal(got["states"][live], ref["states"][live]), (what, "states")


@pytest.mark.parametrize("case", sorted(CASES))
def test_chunked_criterion_run_is_one_long_run(q, orc, case):
    from qecmc import harness
    init, p, H, chunks, ref, kw = _setup(q, orc, case)
    # the carry is exercised, by the oracle's own result
    conv, sd = ref["converged"], ref["steps_done"]
    assert (conv & (sd <= chunks[0])).any(), "no ladder converges inside the first chunk"
    assert (conv & (sd > chunks[0])).any(), "no ladder converges in a later chunk"
    assert (~conv).any(), "no ladder is still running at the horizon"
    print(case, "oracle: converged", int(conv.sum()), "of", len(conv), "first chunk", int((conv & (sd <= chunks[0])).sum()))
    # one launch of the total length
    full = q.pteq_batch(init, p, steps=H, return_states=True, **kw)
    _assert_same(full, ref, "pteq_batch")
    # ... the same run in uneven chunks, and in one chunk through the same entry point (the flags of the live ladders)
    run, one = harness.LadderRun(init, p, **kw), harness.LadderRun(init, p, **kw)
    try:
        snaps, done_at = [], []
        for c in chunks:
            run.advance(c)
            snaps.append(run.snapshot(states=True))
            done_at.append(conv & (sd <= run.steps))
        one.advance(H)
        whole = one.snapshot(states=True)
    finally:
        run.close(); one.close()
    last = snaps[-1]
    assert last["steps"] == H
    _assert_same(last, ref, "chunked")
    _assert_same(whole, ref, "one chunk")
    _assert_same(last, full, "chunked against pteq_batch")
    # (neither the oracle nor pteq_batch returns flags: a flags bug common to both runs shows only through the tops0 and counts of later steps, compared above)
    assert np.array_equal(last["flags"][~conv], whole["flags"][~conv])
    # a ladder that converged in chunk k keeps its rows of all five outputs through every later chunk
    for k, (snap, frozen) in enumerate(zip(snaps, done_at)):
        assert np.array_equal(snap["converged"], frozen), k
        for later in snaps[k + 1:]:
            for key in OUT:
                assert np.array_equal(later[key][frozen], snap[key][frozen]), (k, key)
        for key in OUT:
            assert np.array_equal(snap[key][frozen], ref[key][frozen]), (k, key)
        assert (snap["steps_done"][~frozen] == snap["steps"]).all()


@pytest.mark.parametrize("case", ["toric5", "alpha"])
def test_log_growth_gives_the_same_run(q, orc, case):
    from qecmc import harness
    init, p, H, chunks, ref, kw = _setup(q, orc, case)
    small = harness.LadderRun(init, p, log_rows=3, **kw)
    try:
        small.run_until_converged(H, 211)
        assert small.log_rows >= H > 3 and small.steps == H          # (a ladder is still running at the horizon)
        _assert_same(small.snapshot(states=True), ref, "grown log")
    finally:
        small.close()
    # run_until_converged stops once every ladder has converged: one ladder of the batch on its own (the same Philox index, so the same stop)
    i = int(np.flatnonzero(ref["converged"])[0])
    sd = int(ref["steps_done"][i])
    few = harness.LadderRun(init[i:i + 1], p, **dict(kw, first_syndrome=7 + i))
    try:
        few.run_until_converged(50 * H, 97)
        snap = few.snapshot()
        assert snap["converged"].all() and int(snap["steps_done"][0]) == sd and few.steps == -(-sd // 97) * 97
        for key in OUT:
            assert np.array_equal(snap[key][0], ref[key][i]), key
    finally:
        few.close()


def _buffers(torch, N, Nc, nq, ncls, rec_b, log_b, alpha):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(3)
    mk = lambda n, dt: torch.randint(0, 100, (n,), generator=g, dtype=torch.int32).to(dt).to(dev)
    return dict(states=torch.zeros(N * Nc * nq, dtype=torch.uint8, device=dev), flags=torch.zeros(N * Nc, dtype=torch.uint8, device=dev),
                tops0=mk(N, torch.int32), counts=mk(N * ncls, torch.int32), samples=mk(N, torch.int32), steps_done=mk(N, torch.int32),
                converged=mk(N, torch.uint8), record=torch.zeros(max(rec_b, 1), dtype=torch.uint8, device=dev),
                neff=torch.zeros(N * Nc, dtype=torch.int32, device=dev) if alpha else None,
                log=torch.zeros(max(log_b, 1), dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("kind", ["workspace", "record", "rows", "wave", "colour", "replicas", "none", "null", "neff"])
def test_refusals_launch_nothing(q, kind):
    import torch
    from qecmc import _lib as L_
    N, L, Nc, steps, rows = 100, 5, 5, 50, 80
    kw = dict(code=L_.TORIC, L=L, Nc=Nc, p=0.1, p_logical=0.5, iters=10, steps=steps, tops_burn=0, TOPS=4, SEQ=2, eps=0.3, seed=1,
              conv_mode=L_.CONV_ERROR_BASED)
    kw.update({"wave": dict(scan=L_.SCAN_WAVE), "colour": dict(scan=L_.SCAN_COLOUR), "replicas": dict(replicas=2),
               "none": dict(conv_mode=L_.CONV_NONE)}.get(kind, {}))
    plan = C.c_void_p()
    L_.check(L_.lib().qecmc_plan_create(L_.make_params(**kw), C.byref(plan)))
    try:
        rec, log = C.c_uint64(), C.c_uint64()
        L_.check(L_.lib().qecmc_plan_resume_conv_bytes(plan, N, rows, C.byref(rec), C.byref(log)))
        if kind != "none":
            assert (rec.value, log.value) == (48 * N, 2 * 128 * rows)
        rec_b, log_b = 48 * N, 2 * 128 * rows
        b = _buffers(torch, N, Nc, 2 * L * L, 16, rec_b, log_b, alpha=False)
        before = {k: v.clone() for k, v in b.items() if v is not None}
        step0 = 40 if kind == "rows" else 0                                       # 40 + 50 > 80 rows
        ws_b = log_b - 1 if kind == "workspace" else log_b
        rc_b = rec_b - 1 if kind == "record" else rec_b
        neff = torch.zeros(N * Nc, dtype=torch.int32, device="cuda") if kind == "neff" else None   # not an alpha plan: must be NULL
        rc = L_.lib().qecmc_pteq_resume_conv_dev(
            plan, b["states"].data_ptr(), b["flags"].data_ptr(), b["tops0"].data_ptr(), N, 0, step0, b["counts"].data_ptr(),
            None if kind == "null" else b["samples"].data_ptr(), b["steps_done"].data_ptr(), b["converged"].data_ptr(), b["record"].data_ptr(),
            rc_b, None if neff is None else neff.data_ptr(), b["log"].data_ptr(), ws_b, rows, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = L_.lib().qecmc_last_error().decode()
        print(kind, rc, msg)
        assert rc == (UNSUPPORTED if kind in ("wave", "colour") else INVALID), msg
        assert {"workspace": "workspace", "record": "record", "rows": "rows", "wave": "wave", "colour": "colour", "replicas": "replicas",
                "none": "conv_mode", "null": "NULL", "neff": "d_neff"}[kind] in msg
        torch.cuda.synchronize()
        for k, v in before.items():
            assert torch.equal(b[k], v), k                                         # nothing ran: every buffer is as it was
    finally:
        L_.lib().qecmc_plan_destroy(plan)


@pytest.mark.parametrize("rule", ["PTEQ", "PTEQ_biased", "PTEQ_alpha"])
def test_dropin_continues_instead_of_replaying(q, orc, rule):
    """A one-syndrome drop-in whose ladder outlasts the (shrunk) first horizon: the oracle's percent vector, several launches, no step run twice."""
    from qecmc import decoders
    if rule == "PTEQ":
        code = q.Toric_code(3)
        code.qubit_matrix = _init("toric", 1, 3, 0.1, 8)[0]
        call = lambda: q.PTEQ(code, 0.1, seed=5)
        ref = orc.pteq_batch(orc.TORIC, code.qubit_matrix[None], 0.1, 3, 1 << 21, seed=5, conv_criteria="error_based")
    elif rule == "PTEQ_biased":
        code = q.xzzx_code(3)
        code.qubit_matrix = np.array([[1, 0, 0], [0, 0, 3], [0, 2, 0]], dtype=np.uint8)
        call = lambda: q.PTEQ_biased(code, 0.1, eta=3.0, seed=5)
        ref = orc.pteq_batch(orc.XZZX, code.qubit_matrix[None], 0.1, 3, 1 << 21, seed=5, conv_criteria="error_based", noise=orc.BIASED, eta=3.0)
    else:
        code = q.RotSurCode(3)
        code.qubit_matrix = np.array([[1, 0, 0], [0, 0, 3], [0, 2, 0]], dtype=np.uint8)
        call = lambda: q.PTEQ_alpha(code, 0.1, alpha=1.5, seed=5)
        ref = orc.pteq_batch(orc.ROTATED, code.qubit_matrix[None], 0.1, 3, 1 << 21, seed=5, conv_criteria="error_based", noise=orc.ALPHA, alpha=1.5)
    assert ref["converged"][0] and ref["steps_done"][0] > 64
    exp = (np.divide(ref["counts"][0], ref["samples"][0]) * 100).astype(np.uint8)
    old = decoders.PTEQ_FIRST_HORIZON
    try:
        decoders.PTEQ_FIRST_HORIZON = max(16, int(ref["steps_done"][0]) // 40)
        pct = call()
    finally:
        decoders.PTEQ_FIRST_HORIZON = old
    print(rule, decoders.LAST_RUN, "oracle steps", int(ref["steps_done"][0]))
    assert np.array_equal(pct, exp)
    assert decoders.LAST_RUN["launches"] >= 2 and decoders.LAST_RUN["replayed_steps"] == 0
    assert decoders.LAST_RUN["steps_done"] == int(ref["steps_done"][0])
