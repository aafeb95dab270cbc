"""The (min, +, count) sweep tiled over HBM on the GPU (qecmc_class_minplus_tiled, qecmc_class_minplus_tiled_site): the kernels' costs, counts and
classes equal the host twin's -- the plain loop of csrc/class_minplus_tiled.hpp compiled by g++, which tests/test_class_minplus_tiled_cpu.py pins
against the cut twin, an independent elimination and a sector law -- EXACTLY at the smallest shapes that take each path: fewer entries than a
wavefront, many segments, an odd tile width, holds plus the reduce, rotated L = 13 (the first shape whose state vector does not fit LDS) and rotated
L = 15 (a CLOSE on a fixed slot >= 16).  The tile width changes nothing; with the cut plan's holds the result is qecmc_class_minplus's; syndrome
groups and workspace passes are crossed; the workspace, shared with qecmc_class_sweep_tiled, is reused dirty.  The site form with one table and a row
per syndrome, byte and {0, 1} tables, constant rows, and pure erasure against qecmc_class_sweep_tiled_site.

Beyond the twin's reach -- rotated / xzzx L = 21, planar L = 12, toric L = 7 -- two syndromes each of a few errors: under costs (0, 1, 2, 1) cost
and count are the sector law's (tests/util_minplus_sectors.py), whose counts stay below 2^34 at these chains (asserted: nothing saturates, no pair is
left out); under (0, 1, 1, 1), where no sector law exists, the cost is the slope of log Z_c from qecmc_class_sweep_tiled at two small p against
log(p / 3).  With weights (1, x, x, x), x = p / 3 over 1 - p, Z_c = sum_w N_w x^w and the slope between x1 and x2 is cost + the change of
log(1 + (N_(cost+1) / N_cost) x + ...) per unit of log x, which is below (N_(cost+1) / N_cost) x1.  That ratio is large where the cheapest chains
need a Y in the right place and the next weight does not: at p = 1e-5 and 1e-6 one class of rotated L = 21 showed a slope of 37.934 over a cost of
37, a ratio of about 1e7.  So x1 = 1e-9 and x2 = 1e-10 (p = 3e-9 and 3e-10): a ratio of 1e7 moves the slope by 0.01, and 0.25 is reached only past
2.5e8.  x^40 leaves float64, so all four weights carry one factor s per qubit, the same at both x -- it cancels in the difference of the logarithms
exactly as a common factor of Z -- with s^n_qubits = 1e190: Z_c is about N x^cost 1e190, inside float64 for every cost up to 45 at both x.

Then method "min_weight" of the harness with exact_method="tiled" at rotated L = 13."""
import numpy as np
import pytest

import test_class_minplus_site_cpu as MS
import test_class_minplus_tiled_cpu as MT
import test_class_sweep_tiled_cpu as tiled
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX

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
    return MT.load_twin()


def same(got, want):
    cost, count, cls = want
    assert got["cost"].dtype == np.uint32 and got["count"].dtype == np.uint64 and got["cls"].dtype == np.int32
    assert np.array_equal(got["cost"], cost), (got["cost"], cost)
    assert np.array_equal(got["count"], count), (got["count"], count)
    assert np.array_equal(got["cls"], cls) and np.array_equal(got["saturated"], count == 0)


_L13 = {}


def rotated_L13(T, costs=UNIT):
    """two syndromes at rotated L = 13 and their twin under one cost vector, computed once (shared with the CPU file's elimination test)"""
    if costs not in _L13:
        _L13[costs] = MT.first_shapes_case(T, ROTATED, 13, costs)
    chains, cost, count, cls = _L13[costs]
    return chains, (cost, count, cls)


# ------------------------------------------------------------------------------------------------------ GPU = twin
# (code, L, hbm_width, tile_width, N): a tile of 16 entries -- fewer than a wavefront has lanes, more tiles than entries per lane; a 16-class code
# in many segments; a plaquette code at an odd tile width; holds forced on the torus, with the reduce
@pytest.mark.parametrize("costs", [UNIT, SKEW])
@pytest.mark.parametrize("code,L,hbm_width,tile_width,N", [(XZZX, 5, 0, 4, 5), (TORIC, 3, 0, 6, 3), (ROTATED, 7, 0, 5, 5), (TORIC, 3, 8, 4, 3)])
def test_gpu_equals_host_twin_exactly(q, T, code, L, hbm_width, tile_width, N, costs):
    inf = tiled.info(T, code, L, hbm_width, tile_width)[1]
    chains = MT.chains_of(code, L, N, seed=11)
    got = q.class_minplus_tiled(NAME[code], chains, costs, hbm_width=hbm_width, tile_width=tile_width)
    same(got, MT.twin(T, code, L, chains, costs, hbm_width, tile_width))
    assert (got["held"], got["width"], got["segments"]) == (inf["held"], inf["width"], inf["segments"]) and got["segments"] > 1
    assert (got["held"] > 0) == (hbm_width == 8) and got["count"].min() >= 1
    assert max(sg["n_tiles"] for sg in tiled.segments_of(T, code, L, hbm_width, tile_width)) > 1
    same(q.class_minplus(NAME[code], chains, costs), (got["cost"], got["count"], got["cls"]))         # the cut route takes these shapes too


@pytest.mark.parametrize("costs", MT.COSTS)
def test_rotated_L13_equals_host_twin_exactly(q, T, costs):
    """the first real HBM shape: width 16, 32 tiles of 2^11 per class at the default parameters"""
    chains, want = rotated_L13(T, costs)
    got = q.class_minplus_tiled("rotated", chains, costs)
    same(got, want)
    assert (got["held"], got["width"]) == (0, 16) and len({c.tobytes() for c in want[0]}) == 2


def test_rotated_L15_a_close_on_a_fixed_slot_past_16(q, T):
    assert MT.fixed_slots_closed(T, ROTATED, 15) >= 16
    chains = MT.few_errors(ROTATED, 15, 1, 12, seed=15)                         # (the chain tests/test_class_minplus_tiled_cpu.py ties to the sector law)
    got = q.class_minplus_tiled("rotated", chains, SPLIT)
    same(got, MT.twin(T, ROTATED, 15, chains, SPLIT))
    assert (got["held"], got["width"]) == (0, 18)


def test_the_tile_width_changes_nothing(q, T):
    chains, want = rotated_L13(T)
    one = tuple(w[:1] for w in want)
    same(q.class_minplus_tiled("rotated", chains[:1], UNIT, tile_width=8), one)
    same(q.class_minplus_tiled("rotated", chains[:1], UNIT, tile_width=13), one)


def test_with_the_cut_plans_holds_gpu_is_class_minplus(q):
    chains = MT.chains_of(TORIC, 5, 1, seed=12)
    got = q.class_minplus_tiled("toric", chains, SKEW, hbm_width=13)
    want = q.class_minplus("toric", chains, SKEW, lds_width=13)
    same(got, (want["cost"], want["count"], want["cls"]))
    assert (got["held"], got["width"]) == (want["held"], want["width"]) == (8, 13) and got["count"].min() >= 1


# ------------------------------------------------------------------------------------------------------ boundaries
def test_a_syndrome_group_boundary(q, T):
    """N = 1 030 at 4 classes and nothing held: a group of 1 024 syndromes and one of 6"""
    assert T.qt_class_sweep_cut_group(1030, 4, 0) == 1024
    chains = MT.chains_of(XZZX, 5, 1030, seed=13)
    want = MT.twin(T, XZZX, 5, chains, SKEW, 0, 4)
    same(q.class_minplus_tiled("xzzx", chains, SKEW, tile_width=4), want)
    assert len({a.tobytes() + b.tobytes() for a, b in zip(want[0], want[1])}) > 250          # (many different rows: one in the wrong place would show)


def test_a_workspace_pass_boundary(q, T):
    """rotated L = 17: a state vector of 8 MiB, 128 of them in a pass -- 33 syndromes are 132 units, a pass of 128 and one of 4, the boundary inside a
    syndrome's classes.  The rows repeat three syndromes: equal syndromes give equal rows wherever they fall, the rows of a call of their own -- which
    the sector law gives."""
    assert tiled.info(T, ROTATED, 17)[1]["pass_units"] == 128
    three = MT.few_errors(ROTATED, 17, 3, 10, seed=17)
    alone = q.class_minplus_tiled("rotated", three, SPLIT)
    MT.same_as_law(alone["cost"], alone["count"], *MT.sector_law(ROTATED, 17, three, SPLIT))
    rows = np.arange(33) % 3
    same(q.class_minplus_tiled("rotated", three[rows], SPLIT), (alone["cost"][rows], alone["count"][rows], alone["cls"][rows]))
    assert len({c.tobytes() for c in alone["cost"]}) == 3


def test_a_dirty_workspace_does_not_leak_into_the_next_call(q, T):
    """the workspace is kept per device, never cleared and shared with the sum-product sweep: the same call before and after calls of other shapes,
    widths, tile widths and entry types"""
    chains, want = rotated_L13(T)
    b, c = MT.chains_of(ROTATED, 9, 3, seed=14), MT.chains_of(TORIC, 3, 2, seed=15)
    wb, wc = MT.twin(T, ROTATED, 9, b, SKEW, 0, 8), MT.twin(T, TORIC, 3, c, UNIT, 0, 6)
    w4 = np.array([1.0, 0.043, 0.019, 0.21])
    zs, zcls = tiled.twin(T, ROTATED, 13, chains, w4)
    same(q.class_minplus_tiled("rotated", chains, UNIT), want)
    z = q.class_sweep_tiled("rotated", chains, w4)                              # doubles over the same block
    assert np.array_equal(z["Z"].view(np.uint64), zs.view(np.uint64)) and np.array_equal(z["cls"], zcls)
    same(q.class_minplus_tiled("rotated", b, SKEW, tile_width=8), wb)
    same(q.class_minplus_tiled("toric", c, UNIT, tile_width=6), wc)
    same(q.class_minplus_tiled("rotated", chains, UNIT), want)
    z = q.class_sweep_tiled("rotated", chains, w4)                              # ... and packed entries under the doubles
    assert np.array_equal(z["Z"].view(np.uint64), zs.view(np.uint64))
    same(q.class_minplus_tiled("rotated", b, SKEW, tile_width=8), wb)


# ------------------------------------------------------------------------------------------------------ the site form
@pytest.mark.parametrize("kind", ["bytes", "bits"])
@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4), (XZZX, 5, 0, 4)])
def test_site_gpu_equals_host_twin_with_one_table_and_a_row_per_syndrome(q, T, code, L, hbm_width, tile_width, kind):
    n = 5
    chains = MT.chains_of(code, L, n, seed=16)
    cq = MS.tables_of(code, L, n, kind, seed=16)
    kw = dict(hbm_width=hbm_width, tile_width=tile_width)
    per = q.class_minplus_tiled_site(NAME[code], chains, cq, **kw)
    same(per, MT.site_twin(T, code, L, chains, cq, hbm_width, tile_width))
    same(q.class_minplus_tiled_site(NAME[code], chains, cq[2], **kw), MT.site_twin(T, code, L, chains, cq[2:3], hbm_width, tile_width))
    assert not np.array_equal(per["cost"], q.class_minplus_tiled_site(NAME[code], chains, cq[2], **kw)["cost"])
    if kind == "bits":
        assert (per["count"] > 1).any()                                         # {0, 1} tables tie often


def test_site_rows_cross_a_syndrome_group_boundary(q, T):
    """1 030 rows at 4 classes: the rows of the second group are uploaded on their own and must be the second group's"""
    n = 1030
    chains = MT.chains_of(XZZX, 5, n, seed=17)
    cq = MS.tables_of(XZZX, 5, n, "bytes", seed=17)
    same(q.class_minplus_tiled_site("xzzx", chains, cq, tile_width=4), MT.site_twin(T, XZZX, 5, chains, cq, 0, 4))


@pytest.mark.parametrize("costs", [UNIT, SKEW])
def test_site_constant_rows_equal_the_uniform_entry_point(q, T, costs):
    chains, want = rotated_L13(T, UNIT)
    uniform = q.class_minplus_tiled("rotated", chains, costs)
    for rows in (1, 2):
        cq = np.broadcast_to(np.array(costs, np.uint8), (rows, 13, 13, 4))
        same(q.class_minplus_tiled_site("rotated", chains, cq), (uniform["cost"], uniform["count"], uniform["cls"]))
    if costs == UNIT:
        same(uniform, want)


def test_pure_erasure_at_rotated_L13_against_the_site_sweep(q):
    """Z of qecmc_class_sweep_tiled_site (qecmc.class_sweep_site, method "tiled") under (1, 0, 0, 0) off the erased set counts the chains inside it: non-zero exactly where the class costs 0,
    and then the count"""
    from qecmc import exact as ex
    from qecmc import harness
    rng = np.random.default_rng(1313)
    n = 4
    cells = harness._qubit_cells(ROTATED, 13)
    erased = np.zeros((n,) + cells.shape, bool)
    erased[0, 1, :] = True                                                      # a row and a column: logical operators fit
    erased[0, :, 1] = True
    erased[1:] = rng.random((n - 1,) + cells.shape) < 0.12
    erased &= cells
    assert erased.reshape(n, -1).sum(axis=1).max() <= 40                        # fewer than 4^40 chains in a class... and far fewer with its syndrome
    chains = harness.apply_erasures(np.zeros((n,) + cells.shape, np.uint8), erased, rng)
    got = q.class_minplus_tiled_site("rotated", chains, ex.erasure_site_costs(UNIT, erased))
    z = q.class_sweep_site("rotated", chains, ex.erasure_site_w4(np.array([1.0, 0.0, 0.0, 0.0]), erased), method="tiled")     # qecmc_class_sweep_tiled_site
    assert z["method"] == "tiled"
    assert not got["saturated"].any() and got["count"].max() < 1 << 50
    assert np.array_equal(z["Z"] != 0, got["cost"] == 0) and np.array_equal(z["cls"], got["cls"])
    want = np.where(got["cost"] == 0, got["count"], 0)
    assert np.array_equal(z["Z"], want.astype(np.float64)) and np.array_equal(z["Z"].astype(np.uint64), want)
    assert np.all(got["cost"][np.arange(n), got["cls"]] == 0) and ((got["cost"] == 0).sum(axis=1) > 1).any() and (got["cost"] > 0).any()


# ------------------------------------------------------------------------------------------------------ the top shapes
TOP = [(ROTATED, 21, 6, (0, 24)), (XZZX, 21, 6, (0, 24)), (PLANAR, 12, 6, (0, 24)), (TORIC, 7, 4, (5, 24))]     # (code, L, errors per chain, (held, width))
_top = {}


def top_case(code, L, k):
    """two chains of k errors and the sector law under (0, 1, 2, 1), computed once on the host"""
    if (code, L) not in _top:
        chains = MT.few_errors(code, L, 2, k, seed=L)
        _top[code, L] = (chains,) + MT.sector_law(code, L, chains, SPLIT)
    return _top[code, L]


@pytest.mark.parametrize("code,L,k,plan", TOP)
def test_top_shapes_are_the_sector_law(q, code, L, k, plan):
    chains, want_cost, want_count = top_case(code, L, k)
    limit = 1 << (46 if code == TORIC else 48)
    assert max(int(c) for c in want_count.ravel()) < 1 << 34 < limit            # every (syndrome, class) pair is compared, cost and count
    got = q.class_minplus_tiled(NAME[code], chains, SPLIT)
    assert (got["held"], got["width"]) == plan and not got["saturated"].any()
    MT.same_as_law(got["cost"], got["count"], want_cost, want_count, limit)
    assert np.array_equal(got["cls"], MT.classes(code, chains)) and len(set(got["cost"].ravel().tolist())) > 3


@pytest.mark.parametrize("code,L,k,plan", TOP)
def test_top_shapes_unit_costs_are_the_slope_of_log_z(q, code, L, k, plan):
    from qecmc import harness
    chains = top_case(code, L, k)[0]
    got = q.class_minplus_tiled(NAME[code], chains, UNIT)
    x1, x2 = 1e-9, 1e-10                                                        # p / 3 over 1 - p at p = 3e-9 and 3e-10 (the docstring has the why)
    n_qubits = int(harness._qubit_cells(code, L).sum())
    scale = 10.0 ** (190.0 / n_qubits)
    z1 = q.class_sweep_tiled(NAME[code], chains, scale * np.array([1.0, x1, x1, x1]))["Z"]
    z2 = q.class_sweep_tiled(NAME[code], chains, scale * np.array([1.0, x2, x2, x2]))["Z"]
    assert np.all(z1 > 1e-290) and np.all(z2 > 1e-290) and np.all(z1 < 1e290) and np.all(z2 < 1e290)
    slope = (np.log(z1) - np.log(z2)) / (np.log(x1) - np.log(x2))
    print(NAME[code], L, "slopes", np.round(slope, 4).tolist(), "costs", got["cost"].tolist())
    assert np.abs(slope - np.rint(slope)).max() < 0.25
    assert np.array_equal(got["cost"], np.rint(slope).astype(np.uint32))
    assert np.all(got["cost"] <= top_case(code, L, k)[1])                       # a Y costs 1 here and 2 there


# ------------------------------------------------------------------------------------------------------ method "min_weight" of the harness
def test_harness_min_weight_tiled_is_the_twins_law_at_L13(q, T):
    from qecmc import exact as ex
    from qecmc import harness
    p = 0.03
    errors = harness.draw_errors(ROTATED, 13, 6, p, np.random.default_rng(1301))
    defects = harness.syndrome_of("rotated", errors)
    params = dict(code="rotated", size=13, p_error=p, noise="depolarizing", method="min_weight", exact_method="tiled")
    out = harness.decode_syndromes(params, defects, corrections=True)
    cost, count, cls = MT.twin(T, ROTATED, 13, out["chains"], UNIT)
    assert (count > 0).all()                                                    # the twin reports no saturation at this p_error
    want = ex._law_from_minplus(cost, count, count == 0, (p / 3.0) / (1.0 - p))
    assert out["distr"].shape == (6, 4) and np.array_equal(out["distr"], want) and "counts" not in out
    assert np.array_equal(out["target"], np.argmax(want, axis=1))
    assert np.array_equal(harness.syndrome_of("rotated", out["correction"]), defects)
    assert np.array_equal(np.asarray(harness._class_of(ROTATED, out["correction"])), out["target"])
    with pytest.raises(q.QecmcError, match="qecmc_class_minplus: .*16 generators wide"):            # without the key: the refusal of before
        harness.decode_syndromes(dict(params, exact_method="auto"), defects)
    with pytest.raises(ValueError, match="no traceback"):
        harness.decode_syndromes(dict(params, correction="shortest"), defects, corrections=True)
    gen = harness.generate(dict(params, tile_width=12), 4, seed=5, start="syndrome", corrections=True)
    cost, count, _ = MT.twin(T, ROTATED, 13, gen["qubit_matrix"], UNIT)          # (cost and count are functions of the syndrome: the drawn errors serve)
    assert "counts" not in gen and gen["distr"].dtype == np.float64 and gen["distr"].shape == (4, 4) and (count > 0).all()
    assert np.array_equal(gen["distr"], ex._law_from_minplus(cost, count, count == 0, (p / 3.0) / (1.0 - p)))
    assert np.array_equal(gen["success_correction"], gen["success"])
    era = harness.erasure_experiment(dict(params, p_erase=0.05), 3, seed=7, method="min_weight")
    assert era["distr"].shape == (3, 4) and np.allclose(era["distr"].sum(axis=1), 1.0, atol=1e-12)
    with pytest.raises(q.QecmcError, match="qecmc_class_minplus_site: "):
        harness.erasure_experiment(dict(params, p_erase=0.05, exact_method="cut"), 3, seed=7, method="min_weight")
