"""The six sum-product sweep kernels at the ends of float64's range (qecmc_class_sweep, _cut, _tiled and their _site forms): the rows and the ladder of
tests/test_class_law_range_cpu.py thinned to three values of f per row -- the row's total normal, subnormal and zero -- at the smallest shape each
kernel accepts.  The kernels' Z equal the host twins' as bit patterns, subnormals, zeros and inf included, so what the CPU tests pin on the twins
against the rational law holds for the device; the public law functions refuse and answer on the device exactly where the host path does; and
harness.generate(method="exact") raises the normaliser's FloatingPointError where a tied row's total is about 1e-320.

Every input is a finite weight the entry points accept."""
import numpy as np
import pytest

import test_class_law_range_cpu as R
import test_class_sweep_cpu as S
import test_class_sweep_cut_cpu as SC
import test_class_sweep_site_cpu as SS
import test_class_sweep_tiled_cpu as ST
from qecmc import exact as ex
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX

pytestmark = pytest.mark.gpu

NAME = R.NAME
KW = {"sweep": (), "cut": ("lds_width",), "tiled": ("hbm_width", "tile_width")}
# (route, code, L, widths): the plain sweep with 4 and with 16 classes; the cut sweep's reduce over 2^7 and 2^4 partials; the tiled sweep in tiles of 16
# entries over many segments, with 16 classes, and with five held generators
UNIFORM = [("sweep", ROTATED, 5, ()), ("sweep", TORIC, 3, ()), ("cut", TORIC, 3, (6,)), ("cut", TORIC, 3, (9,)), ("tiled", XZZX, 5, (0, 4)),
           ("tiled", TORIC, 3, (0, 6)), ("tiled", TORIC, 3, (8, 4))]
SITE = [(route, code, widths) for code in (XZZX, ROTATED, PLANAR) for route, widths in R.site_plans(code, 3)]
STEPS = (0, 260, 300)                                                           # of the CPU ladder: totals of 1e-250, 1e-315 and 1e-325


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return SS.load_twin()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def uniform_twin(T, route, code, L, chains, w4, widths):
    return {"sweep": S.twin, "cut": SC.twin, "tiled": ST.twin}[route](T, code, L, chains, w4, *widths)


def outcome(call):
    """("law", the array) or ("refused", the message) of one law function"""
    try:
        return "law", call()
    except FloatingPointError as e:
        return "refused", str(e)


def same_outcome(got, want):
    assert got[0] == want[0], (got, want)
    if got[0] == "law":
        assert np.array_equal(bits(got[1]), bits(want[1]))
    else:
        assert got[1] == want[1] and "row " in got[1]


def ranges_of(z):
    z = np.asarray(z).reshape(-1)
    return {"normal" if v >= 2.0 ** -1022 else "subnormal" if v > 0 else "zero" for v in z.tolist()}


@pytest.mark.parametrize("route,code,L,widths", UNIFORM)
def test_uniform_kernels_equal_the_twins_bit_for_bit_down_the_ladder(q, T, route, code, L, widths):
    case = R.rows_of(T, code, L)
    kw = dict(zip(KW[route], widths))
    run = {"sweep": q.class_sweep, "cut": q.class_sweep_cut, "tiled": q.class_sweep_tiled}[route]
    seen, outcomes = set(), set()
    for k in range(2):
        steps = R.ladder(case["least"][k])
        for p in (steps[s] for s in STEPS):
            w4 = ex.depolarizing_w4(p)
            want, cls = uniform_twin(T, route, code, L, case["chains"], w4, widths)
            got = run(NAME[code], case["chains"], w4, **kw)
            assert got["Z"].dtype == np.float64 and np.array_equal(bits(got["Z"]), bits(want)), (p, got["Z"], want)
            assert np.array_equal(got["cls"], cls)
            seen |= ranges_of(want[k])
            host = outcome(lambda: ex.law_from_class_weights(want))
            same_outcome(outcome(lambda: q.exact_class_probabilities(NAME[code], case["chains"], p, method=route, **kw)), host)
            outcomes.add(host[0])
    assert seen == {"normal", "subnormal", "zero"} and outcomes == {"law", "refused"}


def test_the_enumerators_route_refuses_where_the_host_does(q, T):
    case = R.rows_of(T, ROTATED, 5)
    for p in (R.ladder(case["least"][0])[s] for s in STEPS):
        host = outcome(lambda: ex.exact_class_probabilities("rotated", None, p, hist=case["hist"]))
        same_outcome(outcome(lambda: q.exact_class_probabilities("rotated", case["chains"], p)), host)


@pytest.mark.parametrize("route,code,widths", SITE)
def test_site_kernels_equal_the_twins_bit_for_bit_near_the_bottom(q, T, route, code, widths):
    """the site tables of the CPU tests, one table and one per syndrome"""
    chains = R.rows_of(T, code, 3)["chains"]
    kw = dict(zip(KW[route], widths))
    seen, outcomes = set(), set()
    for wq in [c[0] for c in R.bottom_cases(code)] + [R.bottom_tables(code)[0]]:
        want, cls = SS.twin(T, route, code, 3, chains, wq, widths)
        got = q.class_sweep_site(NAME[code], chains, wq, method=route, **kw)
        assert got["method"] == route and np.array_equal(bits(got["Z"]), bits(want)), (got["Z"], want)
        assert np.array_equal(got["cls"], cls)
        seen |= ranges_of(want)
        host = outcome(lambda: ex.law_from_class_weights(want))
        same_outcome(outcome(lambda: q.exact_site_probabilities(NAME[code], chains, wq, method=route, **kw)), host)
        outcomes.add(host[0])
    assert seen == {"normal", "subnormal", "zero"} and outcomes == {"law", "refused"}


def test_overflow_is_inf_on_the_device_and_refused_by_name(q, T):
    chains = R.rows_of(T, ROTATED, 3)["chains"]
    big = np.array([1e120, 1.0, 1.0, 1.0])
    wq = np.broadcast_to(ex.depolarizing_w4(0.1), (2, 9, 4)).copy()
    wq[1, :, 1:] = 1e40
    for route, widths in R.site_plans(ROTATED, 3):
        kw = dict(zip(KW[route], widths))
        want, _ = uniform_twin(T, route, ROTATED, 3, chains, big, widths)
        got = {"sweep": q.class_sweep, "cut": q.class_sweep_cut, "tiled": q.class_sweep_tiled}[route]("rotated", chains, big, **kw)
        assert np.all(np.isinf(want)) and np.array_equal(bits(got["Z"]), bits(want))
        want, _ = SS.twin(T, route, ROTATED, 3, chains, wq, widths)
        assert np.array_equal(bits(q.class_sweep_site("rotated", chains, wq, method=route, **kw)["Z"]), bits(want)) and np.isinf(want[1]).any()
        with pytest.raises(FloatingPointError, match="row 1: .*overflow"):
            q.exact_site_probabilities("rotated", chains, wq, method=route, **kw)
        with pytest.raises(FloatingPointError, match="row 0: .*overflow"):
            q.exact_site_probabilities("rotated", chains, np.broadcast_to(big, (9, 4)), method=route, **kw)


@pytest.mark.parametrize("exact_method", ["auto", "sweep"])
def test_generate_raises_where_a_tied_rows_total_is_about_1e_320(q, T, exact_method, monkeypatch):
    """rotated L = 5 at the p_error that puts the tied row's total at 1e-320.  At such a p_error no error is ever drawn, so the draw is replaced by
    the tied row: generate hides its class, decodes with method exact and must raise what the host path raises instead of returning a distr"""
    from qecmc import harness
    case = R.rows_of(T, ROTATED, 5)
    p = R.ladder(case["least"][0])[280]
    tied = case["chains"][:1]
    monkeypatch.setattr(harness, "draw_errors", lambda code, size, n, p_error, rng, eta=None, rates=None: np.repeat(tied, n, axis=0))
    if exact_method == "auto":
        host = outcome(lambda: ex.exact_class_probabilities("rotated", None, p, hist=case["hist"][[0, 0, 0]]))
    else:
        host = outcome(lambda: ex.law_from_class_weights(S.twin(T, ROTATED, 5, tied[[0, 0, 0]], ex.depolarizing_w4(p))[0]))
    assert host[0] == "refused" and "row 0" in host[1] and "2^-960" in host[1]
    with pytest.raises(FloatingPointError) as e:
        harness.generate(dict(code="rotated", size=5, p_error=p, noise="depolarizing", method="exact", exact_method=exact_method), 3, seed=5)
    # the histogram is a function of the syndrome, so the enumerator's message is the host's to the letter; the sweep's Z depends on the hidden chain
    # in its last bits, so there the total quoted may differ in its last digit
    head = lambda m: m[:m.index(" total ")]
    assert (str(e.value) == host[1]) if exact_method == "auto" else (head(str(e.value)) == head(host[1]) and "below 2^-960" in str(e.value))
