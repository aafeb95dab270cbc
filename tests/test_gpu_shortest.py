"""qecmc.pteq_shortest_batch: the shortest-chain statistics of PTEQ_alpha_with_shortest (decoders_biasednoise.py:93-172) kept in the kernels of
scan = "wave" and scan = "colour" (csrc/ladder_wu.hpp SHORT, csrc/ladder_colour_body.inc SHORT, csrc/shortest_book.hpp).

Every case runs on both scans and is compared bit for bit, all nine arrays, with the CPU twin of tests/util_shortest_batch.py (level (i): the rule
written out around the oracle's plain ladder); the three percent vectors of qecmc.shortest_distribution with level (ii), the host loop
qecmc.decoders_biasednoise._shortest_loop on the same ladder, the first exactly, the others at rtol = 1e-9 with equal NaN positions (k equal terms
summed one by one against k x term: at most k 2^-53 apart, k <= 2^20).

What makes the cases bite is asserted on the twin before the GPU is asked: ladders leave burn-in, classes hold two and more distinct configurations at
their minimum, minima fall more than once, and the slot's attribute differs from the configuration's own count in many samples (a kernel that recounts
fails); in case A some ladders stop by the criterion and some reach the horizon."""
import numpy as np
import pytest

import util_shortest_batch as U

pytestmark = pytest.mark.gpu

KEYS = ("counts", "samples", "tops0", "steps_done", "converged", "shortest", "shortest_n", "unique_n", "overflow")
SEED, CAP = 31, 1024
# id: code, L, Nc, N, steps, iters, pz_tilde, alpha, criterion (None | dict(eps, TOPS)), tops_burn, first_syndrome
CASES = {
    "A": ("xzzx", 3, 3, 70, 250, 10, 0.3, 2.0, dict(eps=0.6, TOPS=4), 2, 64),       # two wave workgroups, the second ragged; both ways of ending
    "B": ("xzzx", 5, 5, 24, 1500, 10, 0.2, 2.0, None, 1, 128),                      # integer alpha: ties of equal value
    "C": ("rotated", 5, 4, 24, 1200, 7, 0.2, 1.7, None, 1, 0),                      # the general proposal loop, non-integer alpha
    "D": ("rotated", 5, 9, 12, 1500, 10, 0.25, 3.0, dict(eps=0.8, TOPS=4), 2, 0),   # 9 rungs: 1 024-thread workgroups
    "E": ("xzzx", 9, 8, 3, 300, 10, 0.15, 2.5, None, 0, 0),                         # 6 words: the 8-word kernel
    "F": ("xzzx", 7, 7, 4, 400, 10, 0.15, 2.0, None, 0, 0),                         # 4 words exactly
}


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


def twin_args(case, scan):
    code, L, Nc, N, steps, iters, pz, alpha, crit, burn, first = CASES[case]
    c = crit or {}
    return (code, L, Nc, N, steps, iters, pz, alpha, scan, crit is not None, 2, c.get("TOPS", 10), burn, c.get("eps", 0.1), SEED, first)


def run_gpu(q, case, scan, set_capacity=CAP, lo=0, hi=None, first=None, init=None):
    code, L, Nc, N, steps, iters, pz, alpha, crit, burn, first0 = CASES[case]
    init = U.make_init(L, Nc, N) if init is None else init
    kw = dict(conv_criteria="error_based", SEQ=2, **crit) if crit else dict(conv_criteria=None)
    return q.pteq_shortest_batch(init[lo:hi], pz, alpha, Nc=Nc, steps=steps, iters=iters, tops_burn=burn, seed=SEED,
                                 first_syndrome=first0 if first is None else first, code=getattr(q, code.upper()), scan=scan, set_capacity=set_capacity, **kw)


def assert_rows_equal(got, ref, rows=slice(None), what=""):
    for k in KEYS:
        if k == "overflow":
            continue
        print("%s %-10s equal: %s" % (what, k, np.array_equal(got[k][rows], ref[k][rows])))
    for k in KEYS:
        if k != "overflow":
            assert np.array_equal(got[k][rows], ref[k][rows]), (what, k, got[k][rows], ref[k][rows])


@pytest.mark.parametrize("scan", ("wave", "colour"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_shortest_batch_equals_the_twin(q, case, scan):
    ref = U.raw(*twin_args(case, scan))
    N = CASES[case][3]
    # ---- preconditions, on the twin
    assert (ref["samples"] == 0).sum() <= 1, "ladders that never left burn-in"
    if case in "ABCD":
        assert 2 * (ref["unique_n"].max(axis=1) >= 2).sum() >= N
        assert 2 * (ref["falls"] >= 2).sum() >= N
        assert 2 * (ref["stale"] > 0).sum() >= N
    if case == "A":
        assert ref["converged"].sum() == {"wave": 53, "colour": 62}[scan] and N == 70
    if case == "D" and scan == "wave":
        assert ref["converged"].all() and (ref["steps_done"] < 1500).all()
    assert (ref["offered"] <= CAP).all()
    # ---- the kernels
    got = run_gpu(q, case, scan)
    assert set(KEYS) <= set(got)
    assert got["shortest"].dtype == np.float64 and got["shortest"].shape == (N, 4) and got["shortest_n"].dtype == np.uint32 and got["unique_n"].dtype == np.uint32
    assert not got["overflow"].any()
    assert_rows_equal(got, ref, what="%s/%s" % (case, scan))
    if CASES[case][8] is None:
        assert (got["steps_done"] == CASES[case][4]).all() and not got["converged"].any()
    # ---- the reference's three vectors
    a, b, c = q.shortest_distribution(got, CASES[case][6])
    ra, rb, rc = U.triple(*twin_args(case, scan))
    assert a.dtype == np.uint8 and np.array_equal(a, ra)
    np.testing.assert_allclose(b, rb, rtol=1e-9, atol=0, equal_nan=True)
    np.testing.assert_allclose(c, rc, rtol=1e-9, atol=0, equal_nan=True)


@pytest.mark.parametrize("scan", ("wave", "colour"))
def test_a_small_set_overflows_ladder_by_ladder(q, scan):
    """case C with set_capacity = 8: overflow is exactly "the ladder offered more than 8 distinct (configuration, value) pairs"; every other ladder's rows
    stay exact (an overflowed ladder's unique_n row is unspecified, its other rows are not)"""
    ref = U.raw(*twin_args("C", scan))
    want = ref["offered"] > 8
    assert want.any() and not want.all()
    got = run_gpu(q, "C", scan, set_capacity=8)
    assert np.array_equal(got["overflow"], want), (got["overflow"], ref["offered"])
    assert_rows_equal(got, ref, rows=~want, what="overflow/%s" % scan)
    for k in ("counts", "samples", "tops0", "steps_done", "converged", "shortest", "shortest_n"):
        assert np.array_equal(got[k], ref[k]), k
    b = q.shortest_distribution(got, CASES["C"][6])[1]
    assert np.isnan(b[want]).all() and np.array_equal(np.isnan(b[~want]).all(axis=1), ref["samples"][~want] == 0)


@pytest.mark.parametrize("scan", ("wave", "colour"))
def test_sharded_equals_whole(q, scan):
    """Results depend on the global ladder index only (tests/test_gpu_wave.py::test_wave_scan_sharded_equals_whole, on the new arrays).  Case B's 24
    ladders cannot be cut at a multiple of 64, so a full wavefront goes in front of them: 88 ladders of case B's parameters from first_syndrome = 128 in
    one call equal the first 64 from 128 and the last 24 from 192 in two calls."""
    code, L, Nc, _, steps, iters, pz, alpha, _, burn, first = CASES["B"]
    init = U.make_init(L, Nc, 88)
    whole = run_gpu(q, "B", scan, init=init)
    a = run_gpu(q, "B", scan, init=init, hi=64)
    b = run_gpu(q, "B", scan, init=init, lo=64, first=first + 64)
    for k in KEYS:
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]])), k
    assert whole["shortest_n"].sum() > 0 and (whole["unique_n"].max(axis=1) >= 2).sum() >= 44


def test_drop_in_runs_one_syndrome_through_the_kernels(q):
    """PTEQ_alpha_with_shortest(..., scan="colour") equals the host loop on the oracle's scan = 2 ladder"""
    L, Nc, steps, pz, alpha = 5, 5, 600, 0.2, 2.0
    code = q.xzzx_code(L)
    code.qubit_matrix = U.make_init(L, Nc, 1)[0].copy()
    got = q.PTEQ_alpha_with_shortest(code, pz, alpha, Nc=Nc, steps=steps, iters=10, conv_criteria=None, tops_burn=1, scan="colour", seed=77)
    ref = U.triple("xzzx", L, Nc, 1, steps, 10, pz, alpha, "colour", False, 2, 10, 1, 0.1, 77, 0)
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], ref[0][0])
    np.testing.assert_allclose(got[1], ref[1][0], rtol=1e-9, atol=0, equal_nan=True)
    np.testing.assert_allclose(got[2], ref[2][0], rtol=1e-9, atol=0, equal_nan=True)
    assert np.isfinite(ref[1][0]).all() and ref[0][0].sum() > 90


def test_refusals_name_the_case(q):
    init = U.make_init(5, 5, 2)
    kw = dict(Nc=5, steps=50, code=q.XZZX)
    with pytest.raises(q.QecmcError, match="the alpha rule only"):
        q.pteq_shortest_batch(init, 0.1, None, scan="wave", **kw)
    with pytest.raises(q.QecmcError, match="scan = wave or scan = colour"):
        q.pteq_shortest_batch(init, 0.2, 2.0, scan="random", **kw)
    for scan in ("wave", "colour"):
        with pytest.raises(q.QecmcError, match="not with replicas > 1"):
            q.pteq_shortest_batch(init, 0.2, 2.0, scan=scan, replicas=2, **kw)
        with pytest.raises(q.QecmcError, match="not together with qecmc_plan_set_stats"):
            q.pteq_shortest_batch(init, 0.2, 2.0, scan=scan, return_swap_stats=True, **kw)


def test_generate_keeps_the_three_vectors_per_datapoint(q):
    """harness.generate with method "PTEQ_with_shortest" (alpha noise, generate_data.py:167-173): the batched call on the data set's syndromes, the three
    vectors per datapoint, success from the first"""
    from qecmc import harness
    params = dict(code="xzzx", size=5, p_error=0.2, noise="alpha", alpha=2.0, method="PTEQ_with_shortest")
    n, kw = 70, dict(steps=300, conv_criteria=None, tops_burn=1)
    out = harness.generate(params, n, seed=3, **kw)
    rng = np.random.default_rng(3)
    raw = harness.draw_errors(q.XZZX, 5, n, 0.2, rng, None, rates=harness.alpha_rates(0.2, 2.0))
    init = harness.hide_class(q.XZZX, raw, rng)
    res = q.pteq_shortest_batch(init, 0.2, 2.0, Nc=5, seed=3, code=q.XZZX, scan="wave", **kw)
    want = q.shortest_distribution(res, 0.2)
    assert np.array_equal(out["qubit_matrix"], raw) and out["distr"].dtype == np.uint8 and out["distr"].shape == (n, 4)
    for k, w in zip(("distr", "distr_shortest", "distr_shortest_n"), want):
        assert np.array_equal(out[k], w, equal_nan=True), k
    assert np.array_equal(out["success"], np.argmax(out["distr"], axis=1) == out["eq_true"]) and (res["samples"] > 0).sum() > n // 2
    with pytest.raises(ValueError, match="alpha noise"):
        harness.generate(dict(params, noise="depolarizing"), 4, seed=3, **kw)
