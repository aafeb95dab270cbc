"""The traceback on the GPU (qecmc_class_minplus_chains): the kernels' chains, costs, counts and classes equal the host twin's -- the plain loops of
csrc/class_minplus_trace.hpp compiled by g++, which tests/test_class_minplus_trace_cpu.py pins against the oracle and a brute force -- BYTE FOR BYTE:
integer arithmetic and a tie rule that makes the chain a pure function of its inputs, so no order can show.  The shapes are the smallest that reach
each branch of the kernels: part of one ballot word, several words, more h than lanes, the 1 024-thread block, the pick over held generators, a launch
group boundary, the default route at toric L = 5 and the 128 KiB state vector.  Then the cost vectors, the all-zero tie case, dirty memory, cost and
count against qecmc.class_minplus, that entry point against its own twin through the split launch functions, and the harness option."""
import numpy as np
import pytest

import test_class_minplus_cpu as mcpu
import test_class_minplus_trace_cpu as cpu
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
    return random_errors(code, L, n, np.random.default_rng([81, code, L, seed]))


def same(got, want):
    """got: shortest_chains's dict; want: the twin's (chains, cost, count, cls)"""
    out, cost, count, cls = want
    assert got["chains"].dtype == np.uint8 and got["cost"].dtype == np.uint32 and got["count"].dtype == np.uint64 and got["cls"].dtype == np.int32
    assert got["chains"].shape[:2] == cost.shape == got["count"].shape == got["unique"].shape
    assert np.array_equal(got["cost"], cost) and np.array_equal(got["count"], count) and np.array_equal(got["cls"], cls)
    assert np.array_equal(got["chains"].reshape(out.shape), out)
    assert np.array_equal(got["unique"], count == 1) and np.array_equal(got["saturated"], count == 0)


def run_equal(q, T, code, L, n, costs, lds_width=0, seed=0):
    chains = chains_of(code, L, n, seed)
    got = q.shortest_chains(NAME[code], chains, costs, lds_width=lds_width)
    same(got, cpu.twin(T, code, L, chains, costs, lds_width))
    return got


# ------------------------------------------------------------------------------------------------------ (a) the GPU is the twin, branch by branch
# (code, L, lds_width, N, the plan's (width, held))
BRANCHES = [(ROTATED, 3, 0, 5, (4, 0)),          # part of one ballot word: 2^(top - 1) < 64
            (PLANAR, 3, 0, 5, (6, 0)),           # part of one ballot word
            (ROTATED, 5, 0, 5, (8, 0)),          # several ballot words
            (ROTATED, 9, 0, 3, (12, 0)),         # more h than lanes: 2 048 against 256
            (TORIC, 3, 0, 3, (13, 0)),           # the 1 024-thread block
            (TORIC, 3, 6, 3, (6, 7)),            # the pick over 128 partials
            (TORIC, 3, 6, 40, (6, 7)),           # crossing a launch group (32 syndromes)
            (TORIC, 5, 0, 2, (13, 8)),           # the default route
            (ROTATED, 11, 0, 2, (14, 0)),        # the 128 KiB state vector
            (PLANAR, 7, 0, 2, (14, 0))]


@pytest.mark.parametrize("code,L,lds_width,n,plan", BRANCHES)
def test_gpu_equals_host_twin(q, T, code, L, lds_width, n, plan):
    got = run_equal(q, T, code, L, n, cpu.UNIT if (code, L) != (TORIC, 5) else cpu.ALPHA3, lds_width)
    assert (got["width"], got["held"]) == plan
    if n == 40:
        inf = cut.info(T, code, L, lds_width)[1]
        tp = cpu.trace_plan(T, code, L, lds_width)[2]
        assert T.qt_class_minplus_trace_group(n, inf["ncls"], inf["held"], tp["pair_bytes"], None) == 32 < n
        assert len({r.tobytes() for r in got["chains"]}) > 4                    # (many different syndromes: a row in the wrong place would show)


@pytest.mark.parametrize("costs", COSTS)
def test_the_three_cost_vectors_at_rotated_L5(q, T, costs):
    run_equal(q, T, ROTATED, 5, 6, costs, seed=1)


@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 5, 0), (TORIC, 3, 6)])
def test_all_zero_costs_tie_everywhere(q, T, code, L, lds_width):
    """every decision ties and every partial ties: no generator is applied and h* = 0 -- the class representative itself comes back"""
    chains = chains_of(code, L, 4, seed=2)
    got = q.shortest_chains(NAME[code], chains, (0, 0, 0, 0), lds_width=lds_width)
    same(got, cpu.twin(T, code, L, chains, (0, 0, 0, 0), lds_width))
    rows = np.arange(len(chains))
    assert np.all(got["cost"] == 0) and np.array_equal(got["chains"][rows, got["cls"]], chains)


# ------------------------------------------------------------------------------------------------------ (b) dirty memory
def test_dirty_workspace_and_dirty_lds_change_nothing(q, T):
    """0xFF bytes written, freed and handed back to the runtime, then the same call twice with launches of other shapes in between: the pool's blocks
    -- the decision words and the partials among them -- and LDS come back dirty, and the results are the same"""
    import ctypes as C
    hip = q.lib()                                                               # (the handle resolves the HIP runtime the library is linked against)
    block, size = C.c_void_p(), 1 << 29
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t], [C.c_void_p]
    assert hip.hipMalloc(C.byref(block), size) == 0 and hip.hipMemset(block, 0xFF, size) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipFree(block) == 0
    first = run_equal(q, T, ROTATED, 7, 3, cpu.MIXED, seed=3)
    run_equal(q, T, TORIC, 3, 3, cpu.MIXED, 9, seed=3)                          # another shape, held generators, in the same pool blocks
    q.class_sweep_cut("rotated", chains_of(ROTATED, 7, 3, seed=4), np.array([1.0, 0.043, 0.019, 0.21]))      # doubles in the same LDS
    again = run_equal(q, T, ROTATED, 7, 3, cpu.MIXED, seed=3)
    for k in ("chains", "cost", "count", "cls"):
        assert np.array_equal(first[k], again[k]), k
    run_equal(q, T, TORIC, 3, 3, cpu.MIXED, 9, seed=3)


# ------------------------------------------------------------------------------------------------------ (c) next to qecmc.class_minplus
@pytest.mark.parametrize("code,L,lds_width", [(XZZX, 5, 0), (TORIC, 3, 8)])
def test_cost_and_count_are_class_minplus_s(q, code, L, lds_width):
    chains = chains_of(code, L, 5, seed=5)
    got = q.shortest_chains(NAME[code], chains, cpu.ALPHA3, lds_width=lds_width)
    want = q.class_minplus(NAME[code], chains, cpu.ALPHA3, lds_width=lds_width)
    for k in ("cost", "count", "saturated", "cls", "width", "held"):
        assert np.array_equal(got[k], want[k]), k


def test_class_minplus_is_unchanged_through_the_split_launch_functions(q, T):
    chains = chains_of(TORIC, 3, 5, seed=6)
    got = q.class_minplus("toric", chains, cpu.MIXED, lds_width=9)
    cost, count, cls = mcpu.twin(T, TORIC, 3, chains, cpu.MIXED, 9)
    assert np.array_equal(got["cost"], cost) and np.array_equal(got["count"], count) and np.array_equal(got["cls"], cls)


def test_min_weight_corrections(q):
    chains = chains_of(ROTATED, 5, 16, seed=7)
    m = q.min_weight_corrections("rotated", chains)
    r = q.class_minplus("rotated", chains)
    assert np.array_equal(m["target"], q.min_weight_classes("rotated", chains))
    assert np.array_equal(m["weight"], r["cost"].min(axis=1)) and np.array_equal(m["weight"], (m["correction"] != 0).reshape(16, -1).sum(axis=1))


# ------------------------------------------------------------------------------------------------------ (d) the harness
def test_generate_min_weight_with_shortest_corrections(q):
    from qecmc import harness
    params = dict(code="rotated", size=5, p_error=0.1, noise="depolarizing", method="min_weight")
    default = harness.generate(params, 64, seed=9, start="syndrome", corrections=True)
    out = harness.generate(dict(params, correction="shortest"), 64, seed=9, start="syndrome", corrections=True)
    assert np.array_equal(out["qubit_matrix"], default["qubit_matrix"]) and np.array_equal(out["distr"], default["distr"])
    chosen = np.argmax(out["distr"], axis=1)
    cor = out["correction"]
    assert cor.shape == out["qubit_matrix"].shape and cor.dtype == np.uint8
    assert np.array_equal(harness.syndrome_of(q.ROTATED, cor), harness.syndrome_of(q.ROTATED, out["qubit_matrix"]))
    assert np.array_equal(np.asarray(harness._class_of(q.ROTATED, cor)), chosen)
    assert np.array_equal(out["success_correction"], out["success"])            # row by row
    r = q.class_minplus("rotated", out["qubit_matrix"])
    assert np.array_equal(out["correction_weight"], r["cost"][np.arange(64), chosen])           # the least cost of the chosen class
    assert np.array_equal(out["correction_weight"], (cor != 0).reshape(64, -1).sum(axis=1))
    assert np.all(out["correction_weight"] <= default["correction_weight"])      # never heavier than the class move and descent
    print("rows where the traced chain is lighter than the default route's: %d of 64" % int((out["correction_weight"] < default["correction_weight"]).sum()))
    dec = harness.decode_syndromes(dict(params, correction="shortest"), harness.syndrome_of(q.ROTATED, out["qubit_matrix"]), corrections=True)
    assert np.array_equal(dec["correction"], cor) and np.array_equal(dec["target"], chosen) and np.array_equal(dec["correction_weight"], out["correction_weight"])
