"""The site-cost sweep and traceback on the GPU (qecmc_class_minplus_site, qecmc_class_minplus_chains_site): the kernels' costs, counts, classes and
chain bytes equal the host twins' -- the plain loops of csrc/class_minplus_site.hpp compiled by g++, which tests/test_class_minplus_site_cpu.py pins
against an independent elimination and a brute force -- EXACTLY: integer arithmetic and a tie rule that makes the chain a pure function of its
inputs.  The shapes are the smallest that reach each branch of the kernels, each with one table and with a row per syndrome, with random byte tables
and {0, 1} tables.  Then constant rows against the uniform entry points, dirty memory, the pure-erasure tie to the shipped site sweep, and the harness."""
import numpy as np
import pytest

import test_class_minplus_site_cpu as cpu
import test_class_sweep_cut_cpu as cut
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, state_shape

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


def same(sweep, traced, want):
    """sweep: class_minplus_site's dict; traced: shortest_chains_site's; want: the traced twin's (chains, cost, count, cls)"""
    out, cost, count, cls = want
    assert traced["chains"].dtype == np.uint8 and np.array_equal(traced["chains"].reshape(out.shape), out)
    assert np.array_equal(traced["unique"], count == 1)
    for got in (sweep, traced):
        assert got["cost"].dtype == np.uint32 and got["count"].dtype == np.uint64 and got["cls"].dtype == np.int32
        assert np.array_equal(got["cost"], cost) and np.array_equal(got["count"], count) and np.array_equal(got["cls"], cls)
        assert np.array_equal(got["saturated"], count == 0)


def run_equal(q, T, code, L, chains, cq, lds_width=0):
    """both entry points on the GPU against the traced twin (whose cost, count and class the CPU tests pin to the sweep twin's)"""
    rc, msg, out, cost, count, cls = cpu.twin_rc(T, code, L, chains, cq, lds_width)
    assert rc == 0, msg
    sweep = q.class_minplus_site(NAME[code], chains, cq, lds_width=lds_width)
    traced = q.shortest_chains_site(NAME[code], chains, cq, lds_width=lds_width)
    same(sweep, traced, (out, cost, count, cls))
    return sweep, traced


# ------------------------------------------------------------------------------------------------------ (a) the GPU is the twin, branch by branch
# (code, L, lds_width, N, the plan's (width, held))
BRANCHES = [(ROTATED, 3, 0, 5, (4, 0)),          # part of one ballot word: 2^(top - 1) < 64
            (PLANAR, 3, 0, 5, (6, 0)),           # part of one ballot word; cells that hold no qubit
            (ROTATED, 5, 0, 5, (8, 0)),          # several ballot words
            (ROTATED, 9, 0, 3, (12, 0)),         # more states than lanes
            (TORIC, 3, 0, 3, (13, 0)),           # the 1 024-thread block
            (TORIC, 3, 6, 3, (6, 7)),            # the pick over 128 partials
            (TORIC, 3, 6, 40, (6, 7)),           # crossing a launch group (32 syndromes)
            (TORIC, 5, 0, 2, (13, 8)),           # 8 held generators
            (ROTATED, 11, 0, 2, (14, 0)),        # the 128 KiB state vector
            (PLANAR, 7, 0, 2, (14, 0))]


@pytest.mark.parametrize("kind", ["bytes", "bits"])
@pytest.mark.parametrize("rows", ["one", "per"])
@pytest.mark.parametrize("code,L,lds_width,n,plan", BRANCHES)
def test_gpu_equals_host_twin(q, T, code, L, lds_width, n, plan, rows, kind):
    chains = cpu.chains_of(code, L, n, seed=11)
    cq = cpu.tables_of(code, L, 1 if rows == "one" else n, kind, seed=11)
    sweep, traced = run_equal(q, T, code, L, chains, cq, lds_width)
    assert (sweep["width"], sweep["held"]) == plan == (traced["width"], traced["held"])
    if n == 40:
        inf = cut.info(T, code, L, lds_width)[1]
        tp = cpu.MT.trace_plan(T, code, L, lds_width)[2]
        assert T.qt_class_minplus_trace_group(n, inf["ncls"], inf["held"], tp["pair_bytes"], None) == 32 < n
        assert T.qt_class_sweep_cut_group(n, inf["ncls"], inf["held"]) == 32
        if rows == "per":
            assert len({r.tobytes() for r in cq}) == n                          # all rows distinct: a group-local row index used globally would show
            local = np.concatenate([cq[:32], cq[:8]])                           # ... as this table: rows 32 .. 39 replaced by rows 0 .. 7
            assert not np.array_equal(cpu.twin_rc(T, code, L, chains, local, lds_width)[3][32:], sweep["cost"][32:])
    if code == PLANAR and L == 3:
        table = np.broadcast_to(cq.reshape((-1,) + state_shape(code, L) + (4,)), (len(cq), 2, L, L, 4))
        for fill in (0, 255):
            dirty = table.copy()
            dirty[:, 1, -1, :] = fill
            dirty[:, 1, :, -1] = fill
            s2, t2 = run_equal(q, T, code, L, chains, dirty, lds_width)
            for k in ("cost", "count", "cls"):
                assert np.array_equal(s2[k], sweep[k]), k
            assert np.array_equal(t2["chains"], traced["chains"])


# ------------------------------------------------------------------------------------------------------ (b) constant rows
@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 5, 0), (TORIC, 3, 6)])
def test_constant_rows_are_the_uniform_entry_points(q, code, L, lds_width, costs):
    chains = cpu.chains_of(code, L, 5, seed=12)
    cq = np.broadcast_to(np.array(costs, np.uint8), state_shape(code, L) + (4,))
    want_m, want_c = q.class_minplus(NAME[code], chains, costs, lds_width=lds_width), q.shortest_chains(NAME[code], chains, costs, lds_width=lds_width)
    for table in (cq, np.broadcast_to(cq, (5,) + cq.shape)):
        got_m, got_c = q.class_minplus_site(NAME[code], chains, table, lds_width=lds_width), q.shortest_chains_site(NAME[code], chains, table, lds_width=lds_width)
        assert set(got_m) == set(want_m) and set(got_c) == set(want_c)
        for k in want_m:
            assert np.array_equal(got_m[k], want_m[k]), k
        for k in want_c:
            assert np.array_equal(got_c[k], want_c[k]), k


# ------------------------------------------------------------------------------------------------------ (c) dirty memory
def test_dirty_workspace_and_dirty_lds_change_nothing(q, T):
    """0xFF bytes written, freed and handed back to the runtime, then the same call twice with launches of other shapes in between: the pool's blocks
    -- the cost rows, the decision words and the partials among them -- and LDS come back dirty, and the results are the same"""
    import ctypes as C
    hip = q.lib()                                                               # (the handle resolves the HIP runtime the library is linked against)
    block, size = C.c_void_p(), 1 << 29
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t], [C.c_void_p]
    assert hip.hipMalloc(C.byref(block), size) == 0 and hip.hipMemset(block, 0xFF, size) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipFree(block) == 0
    chains, cq = cpu.chains_of(ROTATED, 7, 3, seed=13), cpu.tables_of(ROTATED, 7, 3, "bytes", seed=13)
    other, ocq = cpu.chains_of(TORIC, 3, 3, seed=13), cpu.tables_of(TORIC, 3, 3, "bits", seed=13)
    first = run_equal(q, T, ROTATED, 7, chains, cq)
    run_equal(q, T, TORIC, 3, other, ocq, 9)                                    # another shape, held generators, in the same pool blocks
    q.class_sweep_cut("rotated", chains, np.array([1.0, 0.043, 0.019, 0.21]))   # doubles in the same LDS
    again = run_equal(q, T, ROTATED, 7, chains, cq)
    for a, b in zip(first, again):
        for k in ("cost", "count", "cls"):
            assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(first[1]["chains"], again[1]["chains"])
    run_equal(q, T, TORIC, 3, other, ocq, 9)


# ------------------------------------------------------------------------------------------------------ (d) pure erasure
@pytest.mark.parametrize("code,L", cpu.ERASURE_SHAPES)
def test_pure_erasure_ties_the_kernels_to_the_site_sweep(q, code, L):
    case = cpu.erasure_case(code, L)
    erased = case["erased"]
    lattice = erased[0] if erased[0].ndim == 2 else erased[0, 0]
    assert lattice[1, :].all() and lattice[:, 1].all()                           # a whole row and a whole column of the lattice
    assert erased.reshape(len(erased), -1).sum(axis=1).max() <= 20
    r = q.class_minplus_site(NAME[code], case["chains"], case["cq"])
    z = q.class_sweep_site(NAME[code], case["chains"], q.erasure_site_w4((1, 0, 0, 0), erased))["Z"]
    ranked = q.min_weight_classes_site(NAME[code], case["chains"], case["cq"])
    cpu.check_pure_erasure(z, r["cost"], r["count"], ranked)
    law = q.exact_site_probabilities(NAME[code], case["chains"], q.erasure_site_w4((1, 0, 0, 0), erased))
    assert np.array_equal(ranked, np.argmax(law, axis=1))
    c = q.min_weight_corrections_site(NAME[code], case["chains"], case["cq"])
    assert np.array_equal(c["target"], ranked) and not c["weight"].any()
    assert not c["correction"][~erased].any()                                   # a chain of cost 0 lies inside the erased set


# ------------------------------------------------------------------------------------------------------ (e) the harness
@pytest.mark.parametrize("code,size", [("rotated", 5), ("planar", 4), ("toric", 3)])
def test_erasure_experiment_min_weight_is_the_exact_decoder_at_p_error_0(q, code, size):
    from qecmc import harness
    params = dict(code=code, size=size, p_error=0.0, p_erase=0.25, noise="depolarizing")
    exact = harness.erasure_experiment(params, 24, seed=5)
    short = harness.erasure_experiment(params, 24, seed=5, method="min_weight")
    assert exact["distr"].dtype == short["distr"].dtype == np.float64
    assert np.array_equal(exact["distr"].view(np.uint64), short["distr"].view(np.uint64))     # bit-equal
    for k in ("eq_true", "success", "erased", "chains"):
        assert np.array_equal(exact[k], short[k]), k
    assert np.array_equal(harness.erasure_experiment(params, 24, seed=5, method="exact")["distr"], exact["distr"])
    assert short["success"].any()


def test_generate_min_weight_under_site_costs_with_shortest_corrections(q):
    from qecmc import harness
    n, L = 48, 5
    rng = np.random.default_rng(14)
    cq = rng.integers(0, 4, size=(n, L, L, 4)).astype(np.uint8)
    cq[..., 0] = 0
    params = dict(code="rotated", size=L, p_error=0.1, noise="depolarizing", method="min_weight", site_costs=cq, correction="shortest")
    out = harness.generate(params, n, seed=9, start="syndrome", corrections=True)
    chosen = np.argmax(out["distr"], axis=1)
    cor = out["correction"]
    assert cor.shape == out["qubit_matrix"].shape and cor.dtype == np.uint8
    assert np.array_equal(harness.syndrome_of(q.ROTATED, cor), harness.syndrome_of(q.ROTATED, out["qubit_matrix"]))
    assert np.array_equal(np.asarray(harness._class_of(q.ROTATED, cor)), chosen)
    r = q.class_minplus_site("rotated", out["qubit_matrix"], cq)
    weight = np.take_along_axis(cq.reshape(n, L * L, 4).astype(np.int64), cor.reshape(n, L * L, 1).astype(np.int64), axis=2)[..., 0].sum(axis=1)
    assert np.array_equal(weight, r["cost"][np.arange(n), chosen])              # the correction's weight under the table is the least of its class
    assert np.array_equal(out["distr"], q.shortest_class_law("rotated", out["qubit_matrix"], 0.1, site_costs=cq))
    assert np.array_equal(out["correction_weight"], (cor != 0).reshape(n, -1).sum(axis=1))
    plain = harness.generate(dict(params, site_costs=None, correction=None), n, seed=9, start="syndrome", corrections=True)
    assert np.array_equal(plain["qubit_matrix"], out["qubit_matrix"]) and not np.array_equal(plain["distr"], out["distr"])
    dec = harness.decode_syndromes(params, harness.syndrome_of(q.ROTATED, out["qubit_matrix"]), corrections=True)
    assert np.array_equal(dec["correction"], cor) and np.array_equal(dec["target"], chosen) and np.array_equal(dec["distr"], out["distr"])
