"""A shortest chain of every class on the tiled route, on the GPU (qecmc_class_minplus_tiled_chains, qecmc_class_minplus_tiled_chains_site): the
kernels' chains, costs, counts and classes equal the host twin's -- the plain loop of csrc/class_minplus_tiled_trace.hpp compiled by g++, which knows
nothing of tiles and which tests/test_class_minplus_tiled_trace_cpu.py pins -- BYTE FOR BYTE at the smallest shapes that reach each branch of the
ballot and the gather: 8 half-entries in part of one word with more tiles than entries per lane (xzzx L = 5, tile 4), a 16-class code (toric L = 3,
tile 6), an odd tile and exactly one word (rotated L = 7, tile 5 and 7), two words per tile with one wave looping (tile 8), holds with the pick and
the reduce (toric L = 3, hbm 8, tile 4), rotated L = 13 at the default (four waves, 16 words per tile) and at tile 13 (the 1 024-thread block), and
rotated L = 15 (a CLOSE on a fixed slot >= 16).  The tile width changes nothing.  Where the plan's stream is the cut plan's the chain is
qecmc.shortest_chains' -- a merged kernel and twin that share no code with this path.  A syndrome-group boundary, a workspace-pass boundary, dirty
memory.  Beyond the twin's reach -- rotated / xzzx L = 21, planar L = 12, toric L = 7 -- every chain has the input's syndrome and its class by the
oracle and costs what qecmc.class_minplus_tiled says, which the existing suite pins to the sector law: a complete certificate of a minimum-weight
chain.  The site form; the harness with params['correction'] = "shortest_tiled"."""
import numpy as np
import pytest

import test_class_minplus_site_cpu as MS
import test_class_minplus_tiled_cpu as MT
import test_class_minplus_tiled_trace_cpu as TT
import test_class_sweep_tiled_cpu as tiled
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, state_shape

pytestmark = pytest.mark.gpu

NAME = MT.NAME
UNIT, SPLIT, SKEW = MT.UNIT, MT.SPLIT, (1, 0, 2, 3)                              # SKEW: no two costs equal, a cost of I: a swapped cost shows


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return TT.load_twin()


def same(got, want):
    """the Python layer's dict against the twin's (chains, cost, count, cls), byte for byte"""
    out, cost, count, cls = want
    assert got["chains"].dtype == np.uint8 and got["cost"].dtype == np.uint32 and got["count"].dtype == np.uint64 and got["cls"].dtype == np.int32
    assert np.array_equal(got["cost"], cost), (got["cost"], cost)
    assert np.array_equal(got["count"], count) and np.array_equal(got["cls"], cls) and np.array_equal(got["unique"], count == 1)
    flat = got["chains"].reshape(out.shape)
    assert np.array_equal(flat, out), np.argwhere((flat != out).any(axis=2))[:8].tolist()


def rotated_L13(T, costs=UNIT):
    """two syndromes at rotated L = 13 and the traced twin under one cost vector, computed once (shared with the CPU file)"""
    chains, _, want = TT.first_shapes_case(T, ROTATED, 13, costs)
    return chains, want


# ------------------------------------------------------------------------------------------------------ GPU = twin
SMALL = [(XZZX, 5, 0, 4, 5), (TORIC, 3, 0, 6, 3), (ROTATED, 7, 0, 5, 5), (ROTATED, 7, 0, 7, 5), (ROTATED, 9, 0, 8, 3), (TORIC, 3, 8, 4, 3)]


@pytest.mark.parametrize("costs", [UNIT, SKEW])
@pytest.mark.parametrize("code,L,hbm_width,tile_width,N", SMALL)
def test_gpu_equals_host_twin_byte_for_byte(q, T, code, L, hbm_width, tile_width, N, costs):
    chains = MT.chains_of(code, L, N, seed=21)
    got = q.shortest_chains_tiled(NAME[code], chains, costs, hbm_width=hbm_width, tile_width=tile_width)
    same(got, TT.twin(T, code, L, chains, costs, hbm_width, tile_width))
    plan = TT.trace_plan(T, code, L, hbm_width, tile_width)
    assert (got["held"], got["segments"]) == (plan["held"], plan["segments"]) and got["segments"] > 1 and (got["held"] > 0) == (hbm_width == 8)
    assert plan["words_per_tile"] == (2 if tile_width == 8 else 1)
    assert max(sg["n_tiles"] for sg in tiled.segments_of(T, code, L, hbm_width, tile_width)) > 1


@pytest.mark.parametrize("costs", [UNIT, SKEW])
def test_rotated_L13_equals_host_twin_at_the_default_tile(q, T, costs):
    """the first real HBM shape: width 16, tiles of 2^11 entries, four waves, 16 words per tile and FORGET"""
    chains = rotated_L13(T)[0]
    want = rotated_L13(T)[1] if costs == UNIT else TT.twin(T, ROTATED, 13, chains, costs)
    got = q.shortest_chains_tiled("rotated", chains, costs)
    same(got, want)
    assert (got["held"], got["width"]) == (0, 16) and TT.trace_plan(T, ROTATED, 13)["words_per_tile"] == 16


def test_the_tile_width_changes_nothing(q, T):
    """tile 8 (two words, one wave), 11 and 13 (the 1 024-thread block, 64 words per tile): identical bytes"""
    chains, want = rotated_L13(T)
    for tile_width in (8, 11, 13):
        same(q.shortest_chains_tiled("rotated", chains, UNIT, tile_width=tile_width), want)


def test_rotated_L15_a_close_on_a_fixed_slot_past_16(q, T):
    assert MT.fixed_slots_closed(T, ROTATED, 15) >= 16
    chains, _, want = TT.first_shapes_case(T, ROTATED, 15, SPLIT)
    got = q.shortest_chains_tiled("rotated", chains, SPLIT)
    same(got, want)
    assert (got["held"], got["width"]) == (0, 18)


# ------------------------------------------------------------------------------------------------------ GPU = the cut route's kernels
def test_gpu_is_shortest_chains_where_the_plans_coincide(q):
    for code, L, kw_tiled, kw_cut, n in [(ROTATED, 9, dict(), dict(), 3), (TORIC, 5, dict(hbm_width=13), dict(lds_width=13), 1)]:
        chains = MT.chains_of(code, L, n, seed=22)
        got, want = q.shortest_chains_tiled(NAME[code], chains, SKEW, **kw_tiled), q.shortest_chains(NAME[code], chains, SKEW, **kw_cut)
        for key in ("chains", "cost", "count", "cls", "unique", "saturated"):
            assert np.array_equal(got[key], want[key]), (NAME[code], L, key)
        assert (got["held"], got["width"]) == (want["held"], want["width"])


# ------------------------------------------------------------------------------------------------------ boundaries
def test_a_syndrome_group_boundary(q, T):
    """N = 1 030 at 4 classes and nothing held: a group of 1 024 syndromes and one of 6"""
    assert T.qt_class_sweep_cut_group(1030, 4, 0) == 1024
    few = MT.chains_of(XZZX, 5, 40, seed=23)
    rows = np.arange(1030) % 40
    want = TT.twin(T, XZZX, 5, few, SKEW, 0, 4)
    same(q.shortest_chains_tiled("xzzx", few[rows], SKEW, tile_width=4), tuple(w[rows] for w in want))
    assert len({a.tobytes() for a in want[0]}) > 30                             # (different rows: one in the wrong place would show)


def test_a_workspace_pass_boundary_at_rotated_L13(q, T):
    """2 048 state vectors of width 16 fill the workspace: 513 syndromes are 2 052 pairs, a trace pass of 2 048 and one of 4"""
    plan = TT.trace_plan(T, ROTATED, 13)
    assert T.qt_class_minplus_tiled_trace_pass(plan["state_bits"], plan["pair_bytes"], 2052, 0) == 2048
    chains, want = rotated_L13(T)
    rows = (np.arange(513) * 7 // 5) % 2
    same(q.shortest_chains_tiled("rotated", chains[rows], UNIT), tuple(w[rows] for w in want))


def test_dirty_memory_does_not_leak_into_the_next_call(q, T):
    """the state workspace and the decision block are kept per device and never cleared: call A, then the sum-product sweep and another traced call
    over the same blocks, then A again"""
    chains, want = rotated_L13(T)
    b = MT.chains_of(ROTATED, 9, 3, seed=24)
    wb = TT.twin(T, ROTATED, 9, b, SKEW, 0, 8)
    same(q.shortest_chains_tiled("rotated", chains, UNIT), want)
    q.class_sweep_tiled("rotated", chains, np.array([1.0, 0.043, 0.019, 0.21]))   # doubles over the state vectors
    same(q.shortest_chains_tiled("rotated", b, SKEW, tile_width=8), wb)
    same(q.shortest_chains_tiled("rotated", chains, UNIT), want)
    same(q.shortest_chains_tiled("rotated", b, SKEW, tile_width=8), wb)


# ------------------------------------------------------------------------------------------------------ beyond the twin
TOP = [(ROTATED, 21, 6), (XZZX, 21, 6), (PLANAR, 12, 6), (TORIC, 7, 4)]         # (code, L, errors per chain): tests/test_gpu_class_minplus_tiled.py's


@pytest.mark.parametrize("costs", [UNIT, SPLIT])
@pytest.mark.parametrize("code,L,k", TOP)
def test_top_shapes_chains_are_certified_minimum_weight(q, code, L, k, costs):
    """the chain's syndrome and class by the oracle, and its cost equal to class_minplus_tiled's: no chain of the class is cheaper, and this one is there"""
    chains = MT.few_errors(code, L, 2, k, seed=1)
    got = q.shortest_chains_tiled(NAME[code], chains, costs)
    law = q.class_minplus_tiled(NAME[code], chains, costs)
    assert np.array_equal(got["cost"], law["cost"]) and np.array_equal(got["count"], law["count"]) and np.array_equal(got["cls"], law["cls"])
    TT.check_properties(code, L, chains, costs, got["chains"].reshape(2, got["cost"].shape[1], -1), got["cost"])


@pytest.mark.parametrize("code,L,k", TOP)
def test_top_shapes_unique_rows_are_the_same_from_three_representatives(q, code, L, k):
    """where count == 1 the chain is a function of the syndrome: the chain, the chain times seven generators, and that a logical operator away (one
    syndrome on the torus, whose sixteen classes of 32 assignments make a call the longest of the file)"""
    chains = MT.few_errors(code, L, 2, k, seed=1)[:1 if code == TORIC else 2]
    reps = TT.three_representatives(code, L, chains, 1)
    runs = [q.shortest_chains_tiled(NAME[code], r, UNIT) for r in reps]
    unique = runs[0]["count"] == 1
    assert unique.sum() >= 1
    for again in runs[1:]:
        assert np.array_equal(again["cost"], runs[0]["cost"]) and np.array_equal(again["count"], runs[0]["count"])
        assert np.array_equal(again["chains"][unique], runs[0]["chains"][unique])


# ------------------------------------------------------------------------------------------------------ the site form
@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4), (XZZX, 5, 0, 4)])
def test_site_gpu_equals_host_twin_with_one_table_and_a_row_per_syndrome(q, T, code, L, hbm_width, tile_width):
    n = 5
    chains = MT.chains_of(code, L, n, seed=25)
    for rows in (1, n):
        cq = MS.tables_of(code, L, rows, "bytes", seed=25)
        got = q.shortest_chains_tiled_site(NAME[code], chains, cq.reshape((rows,) + state_shape(code, L) + (4,)), hbm_width=hbm_width, tile_width=tile_width)
        same(got, TT.site_twin(T, code, L, chains, cq, hbm_width, tile_width))


def test_site_rows_at_rotated_L13_and_constant_rows_equal_the_uniform_entry_point(q, T):
    chains, want = rotated_L13(T)
    for costs in (UNIT, SKEW):
        cq = np.broadcast_to(np.array(costs, np.uint8), (1, 13, 13, 4))
        uniform = q.shortest_chains_tiled("rotated", chains, costs)
        site = q.shortest_chains_tiled_site("rotated", chains, cq)
        for key in ("chains", "cost", "count", "cls"):
            assert np.array_equal(site[key], uniform[key]), key
    same(q.shortest_chains_tiled("rotated", chains, UNIT), want)
    cq = MS.tables_of(ROTATED, 13, 2, "bits", seed=26)
    same(q.shortest_chains_tiled_site("rotated", chains, cq.reshape(2, 13, 13, 4)), TT.site_twin(T, ROTATED, 13, chains, cq))


def test_pure_erasure_erased_cells_cost_nothing(q):
    """rotated L = 13 with a third of the cells erased: an erased cell costs 0 whatever it carries, so the chain's cost counts its errors off the set"""
    rng = np.random.default_rng(27)
    erased = rng.random((2, 13, 13)) < 1 / 3
    chains = MT.few_errors(ROTATED, 13, 2, 6, seed=27)
    cq = q.erasure_site_costs(UNIT, erased)
    got = q.shortest_chains_tiled_site("rotated", chains, cq)
    law = q.class_minplus_tiled_site("rotated", chains, cq)
    assert np.array_equal(got["cost"], law["cost"]) and np.array_equal(got["count"], law["count"])
    MS.check_chains(ROTATED, 13, chains, cq.reshape(2, -1, 4), got["chains"].reshape(2, 4, -1), got["cost"])
    off = ((got["chains"] != 0) & ~erased[:, None]).reshape(2, 4, -1).sum(axis=2)
    assert np.array_equal(off, got["cost"])


# ------------------------------------------------------------------------------------------------------ the harness
def test_harness_shortest_tiled_at_rotated_L13(q):
    from qecmc import harness
    n = 8
    params = dict(code="rotated", size=13, p_error=0.05, noise="depolarizing", method="min_weight", exact_method="tiled")
    default = harness.generate(params, n, seed=9, start="syndrome", corrections=True)
    out = harness.generate(dict(params, correction="shortest_tiled"), n, seed=9, start="syndrome", corrections=True)
    assert np.array_equal(out["qubit_matrix"], default["qubit_matrix"]) and np.array_equal(out["distr"], default["distr"])
    chosen = np.argmax(out["distr"], axis=1)
    cor = out["correction"]
    assert cor.shape == out["qubit_matrix"].shape and cor.dtype == np.uint8
    assert np.array_equal(harness.syndrome_of(q.ROTATED, cor), harness.syndrome_of(q.ROTATED, out["qubit_matrix"]))
    assert np.array_equal(np.asarray(harness._class_of(q.ROTATED, cor)), chosen)
    assert np.array_equal(out["success_correction"], out["success"])            # row by row
    r = q.class_minplus_tiled("rotated", out["qubit_matrix"])
    assert np.array_equal(out["correction_weight"], r["cost"][np.arange(n), chosen])            # the least cost of the chosen class
    assert np.array_equal(out["correction_weight"], (cor != 0).reshape(n, -1).sum(axis=1))
    assert np.all(out["correction_weight"] <= default["correction_weight"])      # never heavier than the class move and descent
    print("rows where the traced chain is lighter than the default route's: %d of %d" % (int((out["correction_weight"] < default["correction_weight"]).sum()), n))
    defects = harness.syndrome_of(q.ROTATED, out["qubit_matrix"])
    dec = harness.decode_syndromes(dict(params, correction="shortest_tiled"), defects, corrections=True)
    assert np.array_equal(dec["target"], chosen) and np.array_equal(dec["correction_weight"], out["correction_weight"]) and not dec["correction_source"].any()
    assert np.array_equal(harness.syndrome_of(q.ROTATED, dec["correction"]), defects)
    assert np.array_equal(np.asarray(harness._class_of(q.ROTATED, dec["correction"])), chosen)
    assert np.array_equal(dec["correction_moved"], (chosen != np.asarray(harness._class_of(q.ROTATED, dec["chains"]))).astype(np.uint8))
    unique = r["count"][np.arange(n), chosen] == 1                              # (generate starts from another representative: equal bytes where unique)
    assert np.array_equal(dec["correction"][unique], cor[unique])
    era = harness.erasure_experiment(dict(params, p_erase=0.05, correction="shortest_tiled"), 3, seed=7, method="min_weight")
    assert era["distr"].shape == (3, 4) and np.array_equal(era["target"], np.argmax(era["distr"], axis=1))
    assert np.array_equal(harness.syndrome_of(q.ROTATED, era["correction"]), harness.syndrome_of(q.ROTATED, era["chains"]))
    assert np.array_equal(np.asarray(harness._class_of(q.ROTATED, era["correction"])), era["target"])
    law = q.class_minplus_tiled_site("rotated", era["chains"], q.erasure_site_costs(UNIT, era["erased"]))
    off = ((era["correction"] != 0) & ~era["erased"]).reshape(3, -1).sum(axis=1)   # an erased cell costs nothing
    assert np.array_equal(off, law["cost"][np.arange(3), era["target"]])
