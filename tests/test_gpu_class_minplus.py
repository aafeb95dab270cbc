"""The (min, +, count) sweep on the GPU (qecmc_class_minplus): the kernels' costs, counts and classes equal the host twin's -- the plain loops of
csrc/class_minplus.hpp compiled by g++, which tests/test_class_minplus_cpu.py pins against an independent elimination, the enumerator's histogram and
two sector brute forces -- EXACTLY: integer arithmetic, and a combine that is associative and commutative, so no order can show.  Then held
generators, the 128 KiB state vector, launch-group boundaries, dirty memory, the group count and saturation, the enumerator and the low-p limit of
qecmc.class_sweep on the device, and method "min_weight" of the harness."""
import numpy as np
import pytest

import test_class_minplus_cpu as cpu
import test_class_sweep_cut_cpu as cut
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors

pytestmark = pytest.mark.gpu

NAME = cpu.NAME
COSTS = cpu.COSTS


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return cpu.load_twin()


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([61, code, L, seed]))


def same(got, want):
    """got: class_minplus's dict; want: the twin's (cost, count, cls)"""
    cost, count, cls = want
    assert got["cost"].dtype == np.uint32 and got["count"].dtype == np.uint64 and got["cls"].dtype == np.int32 and got["saturated"].dtype == bool
    assert got["cost"].shape == cost.shape == got["count"].shape == got["saturated"].shape
    assert np.array_equal(got["cost"], cost) and np.array_equal(got["count"], count) and np.array_equal(got["cls"], cls)
    assert np.array_equal(got["saturated"], count == 0)


def run_equal(q, T, code, L, n, costs, lds_width=0, seed=0):
    chains = chains_of(code, L, n, seed)
    got = q.class_minplus(NAME[code], chains, costs, lds_width=lds_width)
    same(got, cpu.twin(T, code, L, chains, costs, lds_width))
    return got


# ------------------------------------------------------------------------------------------------------ (a) the GPU is the twin
EQUAL = [(TORIC, 3), (ROTATED, 3), (ROTATED, 5), (ROTATED, 7), (ROTATED, 9), (XZZX, 9), (PLANAR, 4), (PLANAR, 6)]


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("code,L", EQUAL)
def test_gpu_equals_host_twin(q, T, code, L, costs):
    got = run_equal(q, T, code, L, 5, costs)
    inf = cut.info(T, code, L, 0)[1]
    assert (got["width"], got["held"]) == (inf["width"], inf["held"]) and not got["saturated"].any()


# ------------------------------------------------------------------------------------------------------ (b) held generators
@pytest.mark.parametrize("lds_width", [6, 9, 12])
def test_held_generators_change_nothing_at_toric_L3(q, T, lds_width):
    chains = chains_of(TORIC, 3, 5, seed=1)
    want = q.class_minplus("toric", chains, cpu.MIXED)
    got = q.class_minplus("toric", chains, cpu.MIXED, lds_width=lds_width)
    assert want["held"] == 0 and got["held"] == cut.info(T, TORIC, 3, lds_width)[1]["held"] >= 1 and got["width"] <= lds_width
    for k in ("cost", "count", "cls", "saturated"):
        assert np.array_equal(got[k], want[k]), k
    same(got, cpu.twin(T, TORIC, 3, chains, cpu.MIXED, lds_width))


@pytest.mark.parametrize("lds_width,n", [(13, 2), (14, 1)])
def test_toric_L5_equals_host_twin(q, T, lds_width, n):
    got = run_equal(q, T, TORIC, 5, n, cpu.ALPHA3, lds_width)
    assert (got["held"], got["width"]) == {13: (8, 13), 14: (7, 14)}[lds_width]


# ------------------------------------------------------------------------------------------------------ (c) the 128 KiB state vector
@pytest.mark.parametrize("code,L", [(ROTATED, 11), (PLANAR, 7)])
def test_the_128_KiB_state_vector(q, T, code, L):
    """the dynamic-LDS limit is an attribute of each kernel: k_class_minplus asks for its own"""
    got = run_equal(q, T, code, L, 2, cpu.MIXED)
    assert got["held"] == 0 and got["width"] == 14


# ------------------------------------------------------------------------------------------------------ (d) launch-group boundaries
BOUNDARIES = [(ROTATED, 3, 0, 1027), (TORIC, 3, 6, 35)]


def run_boundary(q, T, code, L, lds_width, n):
    inf = cut.info(T, code, L, lds_width)[1]
    group = T.qt_class_sweep_cut_group(n, inf["ncls"], inf["held"])
    assert group < n                                                            # more than one launch
    got = run_equal(q, T, code, L, n, cpu.UNIT, lds_width, seed=2)
    assert len({r.tobytes() for r in got["count"]}) > 4                         # (many different syndromes: a row in the wrong place would show)
    return group


@pytest.mark.parametrize("code,L,lds_width,n", BOUNDARIES)
def test_launch_group_boundaries(q, T, code, L, lds_width, n):
    group = run_boundary(q, T, code, L, lds_width, n)
    assert group == {1027: 1024, 35: 32}[n]


# ------------------------------------------------------------------------------------------------------ (e) dirty memory
def test_dirty_memory_changes_nothing(q, T):
    """a gibibyte of 0xFF bytes written, freed and handed back to the runtime, and calls with other shapes and numbers of held generators in between:
    the pool's blocks -- the partials among them -- and LDS come back dirty, and the results are the same"""
    import ctypes as C
    hip = q.lib()                                                               # (the handle resolves the HIP runtime the library is linked against)
    block, size = C.c_void_p(), 1 << 30
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t], [C.c_void_p]
    assert hip.hipMalloc(C.byref(block), size) == 0 and hip.hipMemset(block, 0xFF, size) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipFree(block) == 0
    for code, L, lds_width in [(TORIC, 3, 9), (XZZX, 5, 6), (TORIC, 3, 6), (ROTATED, 7, 0), (TORIC, 3, 9)]:
        run_equal(q, T, code, L, 3, cpu.MIXED, lds_width, seed=3)
    q.class_sweep_cut("toric", chains_of(TORIC, 3, 3, seed=3), np.array([1.0, 0.043, 0.019, 0.21]), lds_width=9)   # (doubles in the same pool blocks)
    run_equal(q, T, TORIC, 3, 3, cpu.MIXED, 9, seed=3)
    for code, L, lds_width, n in BOUNDARIES:
        run_boundary(q, T, code, L, lds_width, n)


# ------------------------------------------------------------------------------------------------------ (f) the group count and saturation
def test_all_zero_costs_count_the_group_and_saturate(q):
    r = q.class_minplus("rotated", chains_of(ROTATED, 5, 2), (0, 0, 0, 0))
    assert np.all(r["cost"] == 0) and np.all(r["count"] == 1 << 24) and not r["saturated"].any()
    r = q.class_minplus("toric", chains_of(TORIC, 3, 2), (0, 0, 0, 0))
    assert np.all(r["cost"] == 0) and np.all(r["count"] == 1 << 16)
    chains = chains_of(ROTATED, 7, 2)
    r = q.class_minplus("rotated", chains, (0, 0, 0, 0))                        # 2^48 > kSat
    assert np.all(r["cost"] == 0) and np.all(r["count"] == 0) and r["saturated"].all()
    with pytest.raises(OverflowError, match="row 0"):
        q.exact._law_from_minplus(r["cost"], r["count"], r["saturated"], 0.1)
    assert np.isfinite(q.shortest_class_law("rotated", chains, 0.1)).all()      # (unit costs at the same shape are far from saturation)


# ------------------------------------------------------------------------------------------------------ (g) against the enumerator on the device
@pytest.mark.parametrize("code,L", [(ROTATED, 5), (TORIC, 3)])
def test_gpu_is_the_least_occupied_bin_of_the_enumerator(q, code, L):
    chains = chains_of(code, L, 2, seed=4)
    hist = q.coset_enumerator(NAME[code], chains)["hist"]
    n = np.arange(hist.shape[-1], dtype=np.int64)
    for costs in [cpu.UNIT, cpu.ALPHA3]:
        value = costs[1] * n[:, None] + costs[3] * n[None, :]
        r = q.class_minplus(NAME[code], chains, costs)
        for s in range(len(chains)):
            for c in range(hist.shape[1]):
                occupied = hist[s, c] > 0
                least = value[occupied].min()
                assert (int(r["cost"][s, c]), int(r["count"][s, c])) == (int(least), int(hist[s, c][occupied & (value == least)].sum())), (s, c, costs)


# ------------------------------------------------------------------------------------------------------ (h) the low-p limit of qecmc.class_sweep
@pytest.mark.parametrize("code,L", [(ROTATED, 7), (XZZX, 9)])
def test_low_p_limit_of_class_sweep(q, code, L):
    """count * f^cost against the double sweep's Z at p = 1e-9, relative 1e-5: the CPU test's bound and inputs"""
    chains = random_errors(code, L, 60, np.random.default_rng([52, code, L]))
    r = q.class_minplus(NAME[code], chains)
    z = q.class_sweep(NAME[code], chains, q.depolarizing_w4(cpu.LOW_P))["Z"]
    f = (cpu.LOW_P / 3.0) / (1.0 - cpu.LOW_P)
    want = r["count"].astype(np.float64) * f ** r["cost"].astype(np.float64)
    diff = np.abs(want - z) / z
    print(NAME[code], L, "largest relative difference %.3g, smallest Z %.3g" % (diff.max(), z.min()))
    assert z.min() > 0 and diff.max() <= 1e-5
    law = q.shortest_class_law(NAME[code], chains, cpu.LOW_P)
    assert np.abs(law - z / z.sum(axis=1, keepdims=True)).max() <= 1e-5
    assert np.array_equal(q.min_weight_classes(NAME[code], chains), q.exact._rank_classes(r["cost"], r["count"]))


# ------------------------------------------------------------------------------------------------------ (i) method "min_weight" of the harness
def test_generate_min_weight(q):
    from qecmc import harness
    params = dict(code="rotated", size=5, p_error=0.1, noise="depolarizing", method="min_weight")
    out = harness.generate(params, 64, seed=9)
    assert "counts" not in out and out["distr"].dtype == np.float64 and out["distr"].shape == (64, 4)
    assert np.array_equal(out["distr"], q.shortest_class_law("rotated", out["qubit_matrix"], 0.1))          # row by row: a function of the syndrome
    assert np.array_equal(out["success"], np.argmax(out["distr"], axis=1) == out["eq_true"])
    syn = harness.generate(params, 64, seed=9, start="syndrome", corrections=True)
    assert np.array_equal(syn["qubit_matrix"], out["qubit_matrix"]) and np.array_equal(syn["distr"], out["distr"])
    chosen = np.argmax(syn["distr"], axis=1)
    cor = syn["correction"]
    assert np.array_equal(harness.syndrome_of(q.ROTATED, cor), harness.syndrome_of(q.ROTATED, syn["qubit_matrix"]))
    assert np.array_equal(np.asarray(harness._class_of(q.ROTATED, cor)), chosen)
    r = q.class_minplus("rotated", syn["qubit_matrix"])
    assert np.all(syn["correction_weight"] >= r["cost"][np.arange(64), chosen])
    assert np.array_equal(syn["correction_weight"], (cor != 0).reshape(64, -1).sum(axis=1))
    assert np.array_equal(syn["success_correction"], syn["success"])
    dec = harness.decode_syndromes(params, harness.syndrome_of(q.ROTATED, out["qubit_matrix"]))
    assert np.array_equal(dec["distr"], out["distr"])
    alpha = harness.generate(dict(code="xzzx", size=5, p_error=0.3, noise="alpha", alpha=2, method="min_weight"), 8, seed=3)
    assert np.array_equal(alpha["distr"], q.shortest_class_law("xzzx", alpha["qubit_matrix"], 0.3, alpha=2))
