"""The tiled sweep under site weights on the GPU (qecmc_class_sweep_tiled_site) at the shapes only it reaches, under tables that tell a wrong index
from a right one: the sibling of tests/test_gpu_class_sweep_sectors.py for k_class_sweep_tiled_site, every call through
qecmc.class_sweep_site(..., method="tiled").

Above rotated L = 13 a CLOSE can name a generator whose slot is 16 or higher and lies outside the tile; the kernel decides that pair from the
workgroup's own tile bits (the `fixed` word, 5-bit slots), in a line of its own that the uniform kernel's tests never run.  Here: (a) GPU == site
twin BIT FOR BIT under tables that do not factorise at rotated / xzzx L = 15 and rotated L = 17, with one table and with one per syndrome, after
asserting from the plan that such a CLOSE is in it; (b) planar L = 8 against the twin with NaN in the cells that hold no qubit; (c) the tile width
changes no bit at rotated L = 17 under per-syndrome tables; (d) at rotated / xzzx L = 21, planar L = 12, toric L = 7, planar L = 10 and xzzx L = 17
every class weight against the per-site sector product of tests/util_site_sectors.py, which tests/test_class_sweep_site_sectors_cpu.py pins, one
table per syndrome with a fifth of the qubits erased -- rotated L = 21 with three syndromes crosses a workspace pass inside the call, toric L = 7
with two puts the second row behind 16 classes and 5 held generators; (e) pure erasure at the top shapes, exactly: 0 or powers of two, and
harness.erasure_experiment at rotated L = 15; (f) Z as a function of the syndrome alone under general tables at the top shapes; (g) constant rows
give qecmc.class_sweep_tiled's bits at rotated L = 17.

Tolerance 1e-10 relative in (d) and (f), as tests/test_gpu_class_sweep_sectors.py (d): the sweep errs by about (nq + G) 2^-53 -- 1e-13 at L = 21 --
per partial, sums of non-negative terms throughout; the reference is a sum of non-negative terms over at most 2^16 states and 441 factors per
sector, below 1e-13.  Measured in (d): 2.8e-15 at the worst (rotated L = 21); in (f) the three rows agree bit for bit at both shapes (another
representative permutes a state vector's entries by one XOR pattern, and every op takes the same products and the same pairs to add).  The twin
costs 0.3 s per syndrome at L = 15 and 1.5 s at L = 17, the reference 0.1 - 0.3 s per syndrome, all classes; the whole file takes 15 s."""
import numpy as np
import pytest

import test_class_sweep_cpu as cpu
import test_class_sweep_site_cpu as site
import test_class_sweep_site_sectors_cpu as sectors_cpu
import test_class_sweep_tiled_cpu as tiled
from test_class_sweep_site_sectors_cpu import ERASURE_TOP, HIGH, TOP, assert_high_fixed_close, check_power_of_two_law, general_tables
from test_corrections_cpu import classes, generators
from test_enumerate_cpu import class_chains
from test_gpu_class_sweep_site import same
from test_gpu_class_sweep_tiled import W4, chains_of
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC

pytestmark = pytest.mark.gpu

NAME = cpu.NAME


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return site.load_twin()


def gpu(q, code, chains, wq, tile_width=0):
    got = q.class_sweep_site(NAME[code], chains, wq, method="tiled", tile_width=tile_width)
    assert got["method"] == "tiled"
    return got


_twins = {}


def twin_case(T, code, L, rows, n=2):
    """n syndromes, `rows` general tables and the site tiled twin's answer, computed once: the twin walks the wide stream, whatever the tile"""
    if (code, L, rows, n) not in _twins:
        chains, wq = chains_of(code, L, n), general_tables(code, L, rows)
        want, cls = site.twin(T, "tiled", code, L, chains, wq, (0, 0))
        _twins[code, L, rows, n] = (chains, wq, want, cls)
    return _twins[code, L, rows, n]


# ------------------------------------------------------------------------------------------------------ (a) fixed slots 16 and above
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("tile_width", [0, 8])
@pytest.mark.parametrize("code,L,width", HIGH)
def test_gpu_equals_site_twin_bit_for_bit_where_a_fixed_slot_is_16_or_above(q, T, code, L, width, tile_width, rows):
    assert_high_fixed_close(T, code, L, width, tile_width)                      # the test runs the path it is there for
    chains, wq, want, cls = twin_case(T, code, L, rows)
    got = gpu(q, code, chains, wq, tile_width)
    same(got, want, cls)
    assert (got["held"], got["width"]) == (0, width) and np.all(want > 0) and np.array_equal(cls, classes(code, chains))
    assert all(len(set(z.tolist())) == 4 for z in want) and len({z.tobytes() for z in want}) == 2


# ------------------------------------------------------------------------------------------------------ (b) the planar code
@pytest.mark.parametrize("tile_width", [0, 6])
def test_planar_L8_equals_site_twin_bit_for_bit_with_NaN_in_the_idle_cells(q, T, tile_width):
    """width 16: a shape the LDS sweeps refuse; the cells no generator acts on hold NaN and are read neither by the twin nor on the device"""
    for rows in (1, 3):
        chains, wq, want, cls = twin_case(T, PLANAR, 8, rows, n=3)
        assert np.isnan(wq[:, 1, -1, :]).all() and np.isnan(wq[:, 1, :, -1]).all() and np.isnan(wq).sum() == rows * 15 * 4
        got = gpu(q, PLANAR, chains, wq, tile_width)
        same(got, want, cls)
        assert got["width"] == 16 and got["held"] == 0 and np.all(want > 0) and len({z.tobytes() for z in want}) == 3
    assert cpu.info(T, PLANAR, 8)[0] == -4


# ------------------------------------------------------------------------------------------------------ (c) the tile width at a wide shape
def test_the_tile_width_changes_no_bit_at_rotated_L17_under_per_syndrome_tables(q):
    """tile_width 13 leaves seven fixed bits here, 8 leaves twelve"""
    chains, wq = chains_of(ROTATED, 17, 2, seed=1), general_tables(ROTATED, 17, 2, seed=1)
    want = gpu(q, ROTATED, chains, wq)
    assert want["width"] == 20 and np.all(want["Z"] > 0) and all(len(set(z.tolist())) == 4 for z in want["Z"]) and len({z.tobytes() for z in want["Z"]}) == 2
    for tw in (8, 13):
        same(gpu(q, ROTATED, chains, wq, tw), want["Z"], want["cls"])


# ------------------------------------------------------------------------------------------------------ (d) the independent law
@pytest.mark.parametrize("code,L,n", TOP)
def test_every_class_weight_is_the_site_sector_product(q, T, code, L, n):
    case = sectors_cpu.top_case(code, L)
    chains, wq, want = case["chains"], case["wq"], case["want"]
    inf = q.sweep_tiled_info(NAME[code], L)
    pass_units, units = tiled.info(T, code, L)[1]["pass_units"], n * (inf["ncls"] << inf["held"])
    if (code, L) == (ROTATED, 21):                                              # a pass boundary inside a call whose rows differ
        assert (inf["width"], inf["held"], pass_units, units) == (24, 0, 8, 12) and units > pass_units
    if (code, L) == (TORIC, 7):                                                 # the second row sits behind 16 classes of 2^5 assignments each
        assert (inf["width"], inf["held"], inf["ncls"], n) == (24, 5, 16, 2) and units == 1024 > pass_units
    got = gpu(q, code, chains, wq)
    worst = cpu.rel(got["Z"], want).max()
    print("%s L=%d: %d syndromes x %d classes, width %d, held %d, %d units in passes of %d: worst relative difference %.3g" % (
        NAME[code], L, n, want.shape[1], got["width"], got["held"], units, pass_units, worst))
    assert got["Z"].shape == want.shape == (n, 16 if code == TORIC else 4) and got["width"] > 13
    assert worst < 1e-10
    assert np.array_equal(got["cls"], classes(code, chains))


# ------------------------------------------------------------------------------------------------------ (e) pure erasure
@pytest.mark.parametrize("code,L", sorted(ERASURE_TOP))
def test_pure_erasure_is_exact_at_the_top_shapes(q, code, L):
    """weights (1, 0, 0, 0) off the erased set and (1, 1, 1, 1) on it, the chain uniform on the set: every entry of the state vector is the size of an
    affine set -- 0 or a power of two --, and so is every sum: Z equals the reference exactly"""
    case = sectors_cpu.erasure_top_case(code, L)
    one, several = check_power_of_two_law(case["want"], case["eq_true"])        # on the reference, before the GPU is asked
    assert one >= 1 and several >= 1
    got = gpu(q, code, case["errors"], case["wq"])
    assert np.array_equal(got["Z"], case["want"]) and np.array_equal(got["cls"], case["eq_true"])
    assert check_power_of_two_law(got["Z"], case["eq_true"]) == (one, several)
    assert np.all(got["Z"][np.arange(len(got["Z"])), case["eq_true"]] != 0.0)    # the class of the true chain is never zero


# the seed of that experiment: the first of 0, 1, ... whose eight shots hold one with a single non-zero class and one with several, found on the
# per-site product without a GPU (the test asserts it again)
HARNESS_SEED = 0


def test_erasure_experiment_pure_erasure_at_rotated_L15(q):
    """the harness through the tiled route: the law of every shot is the per-site product's under that shot's erased set, exactly (equal powers of
    two, normalised by the same division), and every shot with a single non-zero class decodes"""
    from qecmc import harness
    out = harness.erasure_experiment(dict(code="rotated", size=15, p_error=0.0, p_erase=0.5, exact_method="tiled"), 8, seed=HARNESS_SEED)
    distr, eq, erased = out["distr"], out["eq_true"], out["erased"]
    assert distr.shape == (8, 4) and erased.shape == (8, 15, 15) and erased.dtype == bool and out["chains"].shape == (8, 15, 15)
    ones = np.ones((15, 15))
    want = np.stack([sectors_cpu.reference(ROTATED, 15, out["chains"][s], ones, erased[s].astype(float), erased[s].astype(float)) for s in range(8)])
    one, several = check_power_of_two_law(want, eq)
    alone = (distr != 0.0).sum(axis=1) == 1
    print("shots with one non-zero class: %d of 8, with several: %d, success rate %.3f" % (one, several, out["success"].mean()))
    assert np.array_equal(distr, want / want.sum(axis=1, keepdims=True))
    assert one >= 1 and several >= 1 and alone.sum() == one and out["success"][alone].all()
    assert np.all(distr[np.arange(8), eq] != 0.0) and np.array_equal(out["success"], np.argmax(distr, axis=1) == eq)


# ------------------------------------------------------------------------------------------------------ (f) Z depends on the syndrome alone
@pytest.mark.parametrize("code,L", [(ROTATED, 21), (TORIC, 7)])
def test_Z_is_a_function_of_the_syndrome_under_general_site_tables(q, code, L):
    """a chain, the chain times a random half of the generators, the chain times a logical operator -- three representatives, so three different CLOSE
    indices on every tile --, each under its own copy of ONE general table: one row of class weights.  No sector law holds for this table."""
    m = sectors_cpu.top_case(code, L)["chains"][0]
    gens, rng = generators(code, L), np.random.default_rng([6, code, L])
    pick = rng.random(len(gens)) < 0.5
    moved = m.ravel() ^ np.bitwise_xor.reduce(gens[pick], axis=0)
    c, ncls = int(classes(code, m[None])[0]), 16 if code == TORIC else 4
    other = class_chains(code, m)[(c + 1) % ncls]
    assert 0.4 * len(gens) < pick.sum() < 0.6 * len(gens) and (moved != m.ravel()).sum() > L and (other != m.ravel()).sum() >= L
    chains = np.stack([m.ravel(), moved, other]).reshape((3,) + m.shape)
    wq = np.repeat(general_tables(code, L, 1, seed=2), 3, axis=0)
    got = gpu(q, code, chains, wq)
    z = got["Z"]
    worst = max(cpu.rel(z[1], z[0]).max(), cpu.rel(z[2], z[0]).max())
    print("%s L=%d: class weights %.3g .. %.3g, worst relative difference between representatives %.3g" % (NAME[code], L, z[0].min(), z[0].max(), worst))
    assert z.shape == (3, ncls) and np.all(z[0] > 1e-200) and len(set(z[0].tolist())) == ncls
    assert worst < 1e-10
    assert got["cls"].tolist() == [c, c, (c + 1) % ncls] and np.array_equal(got["cls"], classes(code, chains))


# ------------------------------------------------------------------------------------------------------ (g) constant rows
def test_constant_rows_are_the_uniform_tiled_sweep_bit_for_bit_at_rotated_L17(q, T):
    assert_high_fixed_close(T, ROTATED, 17, 20)
    chains = chains_of(ROTATED, 17, 2, seed=2)
    uniform = q.class_sweep_tiled("rotated", chains, W4)
    for rows in (1, 2):
        same(gpu(q, ROTATED, chains, np.broadcast_to(W4, (rows, 17, 17, 4))), uniform["Z"], uniform["cls"])
    assert uniform["width"] == 20 and np.all(uniform["Z"] > 0) and len({z.tobytes() for z in uniform["Z"]}) == 2
