"""The exact chain sampler and the exact marginals on the GPU at the bottom of float64's range: the cases of tests/sample_range_cases.py -- the rows and
ladders of tests/test_class_law_range_cpu.py thinned to a normal step, a subnormal one and one past the last positive double, at L = 3, K = 256 --
whose premises tests/test_class_sample_range_cpu.py asserts on the host twins.  The kernels' chains, classes, weights and z equal the twins' byte for
byte, subnormals and zeros included, so what the CPU tests pin on the twins against the rational law holds for the device; every public function
refuses on the device exactly where the host path does, in the same words; the one-chain tables come back as that chain K times, through forced
branches at the last positive double; and none of it depends on what the record and the workspace held before.

The shapes: rotated and xzzx L = 3 with nothing held, toric L = 3 at lds_width = 6, which holds seven generators and takes the pick kernel over
partials and the marginals' combine over held assignments; the four weights, one site table, and one table per syndrome -- the _site kernels."""
import numpy as np
import pytest

import sample_range_cases as RC
import test_class_law_range_cpu as R
import test_class_marginal_cpu as MA
import test_class_sample_cpu as SA
import test_class_sample_range_cpu as cpu
import util_rational_sample as Q
from qecmc import exact as ex
from test_corrections_cpu import generators
from test_gpu_class_law_range import bits, outcome, same_outcome
from test_syndrome_lift_cpu import state_shape

pytestmark = pytest.mark.gpu

NAME = R.NAME
K, SEED = RC.K, RC.SEED


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return MA.load_twin()


def table_of(code, L, wq):
    """a twin's table float[nq, 4] or [N, nq, 4] in the shape the Python layer takes"""
    return None if wq is None else np.asarray(wq).reshape(wq.shape[:-2] + state_shape(code, L) + (4,))


def sampler_equals_twin(q, T, code, L, chains, w, wq, mode, lds_width, K=K):
    """the device against the twin on one call: the same bytes where the twin answers, the same QecmcError where it refuses -> answered"""
    rc, msg, out, cls, z = SA.twin_rc(T, code, L, chains, w=w, wq=wq, K=K, seed=SEED, mode=mode, lds_width=lds_width)
    kw = dict(n_samples=K, seed=SEED, lds_width=lds_width)

    def run():
        if wq is not None:
            return q.sample_posterior(NAME[code], chains, site_weights=table_of(code, L, wq), **kw) if mode else q.sample_chains_site(NAME[code], chains, table_of(code, L, wq), **kw)
        return q.sample_posterior(NAME[code], chains, w4=w, **kw) if mode else q.sample_chains(NAME[code], chains, w4=w, **kw)
    if rc != 0:
        with pytest.raises(q.QecmcError) as e:
            run()
        assert msg in str(e.value) and "row " in msg, (str(e.value), msg)
        return False
    got = run()
    assert np.array_equal(bits(got["z"]), bits(z)), (got["z"], z)
    assert np.array_equal(got["chains"].reshape(out.shape), out)
    if mode:
        assert np.array_equal(got["cls"], cls)
    return True


# ------------------------------------------------------------------------------------------------------ the sampler against the twin
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", RC.CASES, ids=cpu.case_id)
def test_sampler_equals_the_twin_or_refuses_in_its_words(q, T, case, mode):
    code, L, lds_width = case[:3]
    chains, w, wq = cpu.gpu_case_inputs(T, case)
    _, per_class, per_row = RC.premise_of(case)
    # both rows: the first refusal is the twin's; then row 0 alone, whose premise tests/test_class_sample_range_cpu.py asserts
    sampler_equals_twin(q, T, code, L, chains, w, wq, mode, lds_width)
    first = None if wq is None else wq[:1] if wq.ndim == 3 else wq
    assert sampler_equals_twin(q, T, code, L, chains[:1], w, first, mode, lds_width) == (per_row if mode else per_class)


def test_posterior_error_counts_refuses_where_the_sampler_does(q, T):
    case = R.rows_of(T, RC.ROTATED, 3)
    for step, answered in ((0, True), (280, False)):
        p = R.ladder(case["least"][0])[step]
        rc, msg, post, _, _ = SA.twin_rc(T, RC.ROTATED, 3, case["chains"], w=ex.depolarizing_w4(p), K=K, seed=SEED, mode=1)
        assert (rc == 0) == answered
        if answered:
            assert np.array_equal(q.posterior_error_counts("rotated", case["chains"], p, K, seed=SEED), (post != 0).sum(axis=2).mean(axis=1))
        else:
            with pytest.raises(q.QecmcError) as e:
                q.posterior_error_counts("rotated", case["chains"], p, K, seed=SEED)
            assert msg in str(e.value) and "row 0" in msg and "below 2^-960" in msg


# ------------------------------------------------------------------------------------------------------ the marginals against the twin
def flat_answer(res):
    """one float64 array of what a marginal function answers"""
    if isinstance(res, dict):
        return res["marginals"] if "marginals" in res else np.concatenate([res["per_class"].ravel(), res["posterior"].ravel()])
    return res


@pytest.mark.parametrize("case", RC.CASES, ids=cpu.case_id)
def test_marginals_equal_the_twin_and_refuse_where_the_host_path_does(q, T, case, monkeypatch):
    code, L, lds_width, ladder, step, form = case
    chains, w, wq = cpu.gpu_case_inputs(T, case)
    table = table_of(code, L, wq)
    out, z, cls = MA.twin(T, code, L, chains, w=w, wq=wq, lds_width=lds_width)
    raw = q.class_marginals(NAME[code], chains, w4=w, lds_width=lds_width, normalize=False) if wq is None else \
        q.class_marginals_site(NAME[code], chains, table, lds_width=lds_width, normalize=False)
    assert np.array_equal(bits(raw["z"]), bits(z)), (raw["z"], z)               # as bit patterns: subnormals and zeros included
    assert np.array_equal(bits(raw["weights"]).reshape(-1), bits(out).reshape(-1)) and np.array_equal(raw["cls"], cls) and "marginals" not in raw
    assert RC.ranges_of(z[0]) == RC.premise_of(case)[0]
    calls = [lambda: ex.class_marginals(NAME[code], chains, w4=w, lds_width=lds_width) if wq is None else ex.class_marginals_site(NAME[code], chains, table, lds_width=lds_width),
             lambda: ex.posterior_marginals(NAME[code], chains, lds_width=lds_width, **(dict(w4=w) if wq is None else dict(site_weights=table)))]
    if form == "w4":
        rows = R.rows_of(T, code, L)
        p = {"row": R.ladder(rows["least"][0]), "class": cpu.class_ladder(rows, 0)}[ladder][step]
        assert np.array_equal(ex.depolarizing_w4(p), w)
        calls.append(lambda: ex.exact_error_counts(NAME[code], chains, p, lds_width=lds_width))
    with monkeypatch.context() as m:                                            # the host path: the twin's numbers through the same normalising code
        m.setattr(ex, "_marginals", cpu.through_the_twin(T, L))
        host = [outcome(lambda: flat_answer(call())) for call in calls]
    for call, want in zip(calls, host):
        same_outcome(outcome(lambda: flat_answer(call())), want)


def test_the_cases_cross_both_outcomes_of_every_function(T):
    """the premises again, from the data module alone: every function of either kind both answers and refuses over the cases"""
    for which in (1, 2):
        assert {RC.premise_of(c)[which] for c in RC.CASES} == {True, False}
    assert set().union(*(RC.premise_of(c)[0] for c in RC.CASES)) == {"normal", "subnormal", "zero"}


# ------------------------------------------------------------------------------------------------------ one-chain tables on the device
@pytest.mark.parametrize("code,L,lds_width", RC.SHAPES)
def test_one_chain_tables_on_the_device(q, T, code, L, lds_width):
    """2^-299 and 2^-955 are answered with that chain K times; 2^-1000 and the last positive double are refused in the twin's words; the mixed table
    of the CPU tests is answered through forced branches at s = 2^-1074"""
    chain = R.rows_of(T, code, L)["chains"][1]
    gens = generators(code, L)
    flat = cpu.far_chain(gens, chain)
    for e, answered in ((299, True), (955, True), (1000, False), (1074, False)):
        tab = Q.one_chain_table(gens, flat, 2.0 ** -e)
        assert sampler_equals_twin(q, T, code, L, chain[None], None, tab, 1, lds_width) == answered
        if answered:
            got = q.sample_posterior(NAME[code], chain[None], site_weights=table_of(code, L, tab), n_samples=K, seed=SEED, lds_width=lds_width)
            assert (got["chains"].reshape(K, -1) == flat).all() and len(np.unique(got["cls"])) == 1 and got["z"][0, got["cls"][0, 0]] == 2.0 ** -e
    start, one, tab = cpu.mixed_one_chain_table(T, code, L, lds_width)
    assert sampler_equals_twin(q, T, code, L, start[None], None, tab, 1, lds_width)
    got = q.sample_posterior(NAME[code], start[None], site_weights=table_of(code, L, tab), n_samples=K, seed=SEED, lds_width=lds_width)
    assert (got["chains"].reshape(K, -1) == one).all() and got["z"][0].max() == 2.0 ** -950
    raw = q.class_marginals_site(NAME[code], start[None], table_of(code, L, tab), lds_width=lds_width, normalize=False)
    out, z, _ = MA.twin(T, code, L, start[None], wq=tab, lds_width=lds_width)
    assert np.array_equal(bits(raw["weights"]).reshape(-1), bits(out).reshape(-1)) and np.array_equal(bits(raw["z"]), bits(z))


# ------------------------------------------------------------------------------------------------------ dirty memory
def test_dirty_record_and_workspace_change_nothing_at_the_bottom(q, T):
    """0xFF bytes written, freed and handed back to the runtime, then the widest call of the file -- toric L = 3 at lds_width = 6, both families --,
    then the subnormal steps: the record, the partials, the forward record of the marginals and LDS come back dirty, and the bytes are the twin's"""
    import ctypes as C
    hip = q.lib()                                                               # (the handle resolves the HIP runtime the library is linked against)
    block, size = C.c_void_p(), 1 << 29
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t], [C.c_void_p]
    assert hip.hipMalloc(C.byref(block), size) == 0 and hip.hipMemset(block, 0xFF, size) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipFree(block) == 0
    wide = (RC.TORIC, 3, 6, "class", 0, "w4")
    chains, w, _ = cpu.gpu_case_inputs(T, wide)
    assert sampler_equals_twin(q, T, RC.TORIC, 3, chains, w, None, 0, 6)
    q.class_marginals("toric", chains, w4=w, lds_width=6, normalize=False)
    for code in (RC.ROTATED, RC.XZZX):
        start, one, tab = cpu.mixed_one_chain_table(T, code, 3, 0)             # pairs at the last positive double in an answered call
        assert sampler_equals_twin(q, T, code, 3, start[None], None, tab, 1, 0)
        for ladder, step, mode in (("class", 260, 1), ("row", 260, 1), ("row", 300, 0)):
            chains, w, wq = cpu.gpu_case_inputs(T, (code, 3, 0, ladder, step, "rows"))
            sampler_equals_twin(q, T, code, 3, chains, w, wq, mode, 0)
            out, z, _ = MA.twin(T, code, 3, chains, wq=wq)
            raw = q.class_marginals_site(NAME[code], chains, table_of(code, 3, wq), normalize=False)
            assert np.array_equal(bits(raw["weights"]).reshape(-1), bits(out).reshape(-1)) and np.array_equal(bits(raw["z"]), bits(z))
