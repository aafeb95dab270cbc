"""The three sweeps under a weight per (syndrome, qubit) on the GPU (qecmc_class_sweep_site, _cut_site, _tiled_site): the kernels' class weights equal
the host twins' -- the plain loops of csrc/class_sweep_site.hpp compiled by g++, which tests/test_class_sweep_site_cpu.py pins against an
independent elimination -- BIT FOR BIT, with one table and with one per syndrome, at the smallest shapes that take each path: the LDS sweep with 16
and with 4 classes and with cells that hold no qubit; the cut sweep with ten and eight held generators and on the 128 KiB state vector; the tiled
sweep with CLOSE pairs on fixed slots, with held generators and at rotated L = 13.  Constant rows give the uniform entry points' bits.  Launch
groups and workspace passes are crossed with per-syndrome tables: a row offset that forgets the group's first syndrome, or a pass's first unit,
reads another shot's weights.  The pure-erasure channel is exact on the device.  Then the harness: erasure_experiment at rotated L = 5.

The tiled pass boundary: at the small plan of the CPU tests (xzzx L = 5, tiles of 2^4) a launch group is 1 024 syndromes of 4 units and a pass takes
65 535 units, so no N needs two passes there; that plan crosses a group boundary (N = 1 025).  Two passes are crossed at the smallest plan that has
them: toric L = 3 with hbm_width 8 -- 512 units per syndrome, groups of 128 syndromes, 65 536 units: a pass of 65 535 and one of 1.

Tolerance of test 6 against util_site.eliminate_site: 1e-12 on the normalised law, as the CPU tests' -- either side errs by about (nq + G) 2^-53."""
import numpy as np
import pytest

import test_class_sweep_cut_cpu as cut
import test_class_sweep_site_cpu as site
import test_class_sweep_tiled_cpu as tiled
from test_corrections_cpu import generators
from test_enumerate_cpu import class_chains
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX
from util_site import eliminate_site

pytestmark = pytest.mark.gpu

NAME = site.NAME
# 1: (route, code, L, widths)
EQUAL = [("sweep", TORIC, 3, ()), ("sweep", PLANAR, 4, ()), ("sweep", XZZX, 5, ()), ("cut", TORIC, 3, (4,)), ("cut", TORIC, 5, (13,)), ("cut", ROTATED, 11, (0,)),
         ("tiled",) + site.SMALL_TILED[:2] + (site.SMALL_TILED[2:],), ("tiled",) + site.HELD_TILED[:2] + (site.HELD_TILED[2:],), ("tiled", ROTATED, 13, (0, 0))]
# 3: (route, code, L, widths, N)
BOUNDARIES = [("sweep", XZZX, 3, (), 1025), ("cut", TORIC, 3, (4,), 5), ("tiled",) + site.SMALL_TILED[:2] + (site.SMALL_TILED[2:], 1025),
              ("tiled",) + site.HELD_TILED[:2] + (site.HELD_TILED[2:], 129)]


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return site.load_twin()


def same(got, want_z, want_cls):
    assert got["Z"].dtype == np.float64 and got["Z"].shape == want_z.shape
    assert np.array_equal(got["Z"].view(np.uint64), want_z.view(np.uint64))
    assert got["cls"].dtype == np.int32 and np.array_equal(got["cls"], want_cls)


def gpu(q, route, code, chains, wq, widths):
    kw = dict(zip({"sweep": (), "cut": ("lds_width",), "tiled": ("hbm_width", "tile_width")}[route], widths))
    got = q.class_sweep_site(NAME[code], chains, wq, method=route, **kw)
    assert got["method"] == route
    return got


_cases = {}


def case(T, route, code, L, widths, n, rows):
    """chains, tables and the twin's answer of one case, computed once (the dirty-memory test runs every case again)"""
    key = (route, code, L, tuple(widths), n, rows)
    if key not in _cases:
        chains, wq = site.chains_of(code, L, n, seed=len(widths)), site.tables_of(code, L, rows, seed=n)
        want, cls = site.twin(T, route, code, L, chains, wq, widths)
        _cases[key] = (chains, wq, want, cls)
    return _cases[key]


def run_equal(q, T, route, code, L, widths, rows):
    chains, wq, want, cls = case(T, route, code, L, widths, 3, rows)
    got = gpu(q, route, code, chains, wq if rows == 3 else wq[0], widths)
    same(got, want, cls)
    assert np.all(want > 0) and len({z.tobytes() for z in want}) == 3
    return got


def run_boundary(q, T, route, code, L, widths, n):
    chains, wq, want, cls = case(T, route, code, L, widths, n, n)
    same(gpu(q, route, code, chains, wq, widths), want, cls)
    assert len({z.tobytes() for z in want}) == n                                # (every row has its own table: a row in the wrong place would show)


# ------------------------------------------------------------------------------------------------------ 1. the kernels against the twins
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("route,code,L,widths", EQUAL)
def test_gpu_equals_site_twin_bit_for_bit(q, T, route, code, L, widths, rows):
    got = run_equal(q, T, route, code, L, widths, rows)
    inf = {"sweep": lambda: dict(site.S.info(T, code, L)[1], held=0), "cut": lambda: cut.info(T, code, L, *widths)[1],
           "tiled": lambda: tiled.info(T, code, L, *widths)[1]}[route]()
    assert (got["width"], got["held"]) == (inf["width"], inf["held"])
    if (route, code, L) == ("cut", ROTATED, 11):
        assert (got["width"], got["held"]) == (14, 0)                           # the 128 KiB state vector
    if (route, code, L) == ("cut", TORIC, 5):
        assert (got["width"], got["held"]) == (13, 8)


# ------------------------------------------------------------------------------------------------------ 2. constant rows
@pytest.mark.parametrize("route,code,L,widths", [("sweep", PLANAR, 4, ()), ("cut", TORIC, 3, (4,)), ("tiled",) + site.SMALL_TILED[:2] + (site.SMALL_TILED[2:],)])
def test_constant_rows_are_the_uniform_entry_point_bit_for_bit(q, route, code, L, widths):
    chains = site.chains_of(code, L, 3, seed=5)
    uniform = {"sweep": lambda: q.class_sweep(NAME[code], chains, site.W4), "cut": lambda: q.class_sweep_cut(NAME[code], chains, site.W4, lds_width=widths[0]),
               "tiled": lambda: q.class_sweep_tiled(NAME[code], chains, site.W4, hbm_width=widths[0], tile_width=widths[1])}[route]()
    for rows in (1, 3):
        same(gpu(q, route, code, chains, np.broadcast_to(site.W4, (rows, site.nq_of(code, L), 4)), widths), uniform["Z"], uniform["cls"])
    assert np.all(uniform["Z"] > 0)


def test_constant_rows_give_the_law_of_the_uniform_entry_points(q):
    site.test_constant_rows_give_the_law_of_the_uniform_entry_points()


# ------------------------------------------------------------------------------------------------------ 3. groups and passes
@pytest.mark.parametrize("route,code,L,widths,n", BOUNDARIES)
def test_group_and_pass_boundaries(q, T, route, code, L, widths, n):
    if route == "sweep":
        assert n == 1024 + 1                                                    # sweep::kGroupMax + 1
    else:
        inf = (cut.info(T, code, L, *widths) if route == "cut" else tiled.info(T, code, L, *widths))[1]
        group = T.qt_class_sweep_cut_group(10 ** 6, inf["ncls"], inf["held"])
        assert n == group + 1
        if (code, L) + tuple(widths) == site.HELD_TILED:                        # ... and the first group takes two passes
            assert group * (inf["ncls"] << inf["held"]) == inf["pass_units"] + 1
    run_boundary(q, T, route, code, L, widths, n)


# ------------------------------------------------------------------------------------------------------ 4. zero weights
def test_pure_erasure_is_exact_on_the_device(q, T):
    c = site.erasure_case(T, ROTATED, 5)
    want, cls = site.twin(T, "sweep", ROTATED, 5, c["chains"], c["wq"])
    got = q.class_sweep_site("rotated", c["chains"], c["wq"])
    same(got, want, cls)
    one, several = site.check_erasure_law(got["Z"], c["eq_true"])
    assert got["method"] == "sweep" and one >= 5 and several >= 1
    for route, kw in (("cut", dict(lds_width=5)), ("tiled", dict(tile_width=4))):          # the other routes: the same counts, exactly
        other = q.class_sweep_site("rotated", c["chains"], c["wq"], method=route, **kw)
        assert np.array_equal(other["Z"], got["Z"]) and other["method"] == route


# ------------------------------------------------------------------------------------------------------ 5, 6. the harness
def test_erasure_experiment_pure_erasure(q):
    from qecmc import harness
    out = harness.erasure_experiment(dict(code="rotated", size=5, p_error=0.0, p_erase=0.25), 64, seed=3)
    distr, eq = out["distr"], out["eq_true"]
    assert distr.shape == (64, 4) and out["erased"].shape == (64, 5, 5) and out["erased"].dtype == bool and out["chains"].shape == (64, 5, 5)
    assert np.allclose(distr.sum(axis=1), 1.0, atol=1e-12)
    alone = (distr != 0.0).sum(axis=1) == 1
    print("shots with one non-zero class: %d of 64, success rate %.3f" % (alone.sum(), out["success"].mean()))
    assert alone.sum() >= 32 and out["success"][alone].all()
    assert np.all(distr[np.arange(64), eq] != 0.0)
    assert np.array_equal(out["success"], np.argmax(distr, axis=1) == eq)


def test_erasure_experiment_is_the_elimination_under_erasure_weights(q):
    from qecmc import exact as ex
    from qecmc import harness
    out = harness.erasure_experiment(dict(code="rotated", size=5, p_error=0.05, p_erase=0.25), 8, seed=4)
    wq = ex.erasure_site_w4(ex.depolarizing_w4(0.05), out["erased"]).reshape(8, 25, 4)
    gens = generators(ROTATED, 5)
    assert out["erased"].any() and not out["erased"].all()
    for s in range(8):
        z = np.array([eliminate_site(gens, r, wq[s]) for r in class_chains(ROTATED, out["chains"][s])])
        assert np.abs(out["distr"][s] - z / z.sum()).max() < 1e-12
    assert np.array_equal(out["success"], np.argmax(out["distr"], axis=1) == out["eq_true"])


# ------------------------------------------------------------------------------------------------------ 7. dirty memory
def test_dirty_memory_changes_no_bit(q, T):
    """a gibibyte of 0xFF bytes -- NaNs as doubles, out-of-range indices as words -- written, freed and handed back to the runtime; then every case of tests
    1 and 3 once more: the device blocks, the tiled workspace and LDS come back dirty, and the results are the same bits"""
    import ctypes as C
    hip = q.lib()                                                               # (the handle resolves the HIP runtime the library is linked against)
    block, size = C.c_void_p(), 1 << 30
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t], [C.c_void_p]
    assert hip.hipMalloc(C.byref(block), size) == 0 and hip.hipMemset(block, 0xFF, size) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipFree(block) == 0
    for route, code, L, widths in EQUAL:
        for rows in (1, 3):
            run_equal(q, T, route, code, L, widths, rows)
    for route, code, L, widths, n in BOUNDARIES:
        run_boundary(q, T, route, code, L, widths, n)
