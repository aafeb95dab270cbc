"""The per-site sector product of tests/util_site_sectors.py, without a GPU: pinned here before tests/test_gpu_class_sweep_site_sectors.py lets it
judge the tiled sweep under site weights at the shapes no host twin reaches (rotated / xzzx L = 21, planar L = 12, toric L = 7).

What is pinned: the product equals a brute force over the whole group at L = 3 for every code and class under random per-qubit rows with erased
cells; it equals util_site.eliminate_site on the whole lattice at rotated / xzzx L = 5, planar L = 4 and toric L = 3; it equals the site twins of
csrc/class_sweep_site.hpp on all three routes, with one table and with one per syndrome; it equals the site tiled twin at rotated / xzzx L = 15 and
rotated L = 17, where a CLOSE names a fixed slot of 16 or above (asserted from the plan) -- the pair the twin decides by `pr & 31u`, which no other
CPU test reaches; the cells that hold no qubit carry NaN throughout and are not read by either side; the reference cases of the GPU test are
finite, far above the underflow, and tell classes and syndromes apart; the pure-erasure references are 0 or powers of two.

Tolerance 1e-12 relative per class weight, as tests/test_class_sweep_sectors_cpu.py: either side is a sum of non-negative terms and errs by about
(nq + G) 2^-53 -- 1e-13 at L = 21; the table's w_Y = c fx fz is rounded once more per qubit, which the same figure covers.  Measured: at most
1.3e-15 (the tiled twin at rotated L = 13).  The reference costs 0.1 - 0.3 s per syndrome, all classes, at the top shapes; the file takes 20 s."""
import numpy as np
import pytest

import test_class_sweep_cpu as S
import test_class_sweep_site_cpu as site
import test_class_sweep_tiled_cpu as tiled
import util_sectors as U
import util_site_sectors as US
from test_class_sweep_sectors_cpu import table
from test_corrections_cpu import classes, generators
from test_enumerate_cpu import class_chains, span
from test_gpu_class_sweep_sectors import closes_on_high_fixed_slots          # (plan inspection alone: it imports without a GPU)
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_site import eliminate_site

NAME = S.NAME
# (code, L, syndromes): where tests/test_gpu_class_sweep_site_sectors.py holds the tiled site sweep against the product.  Rotated L = 21 with three
# syndromes does not fit one workspace pass; toric L = 7 with two puts a second table row behind 16 classes and 5 held generators
TOP = [(ROTATED, 21, 3), (XZZX, 21, 2), (PLANAR, 12, 2), (TORIC, 7, 2), (PLANAR, 10, 2), (XZZX, 17, 2)]
# (code, L, tile_width -> width): the shapes whose plan closes a pair on a fixed slot >= 16
HIGH = [(ROTATED, 15, 18), (XZZX, 15, 18), (ROTATED, 17, 20)]
# (route, code, L, widths): where a site twin is cheap
TWINS = [("sweep", XZZX, 9, ()), ("cut", ROTATED, 11, (0,)), ("cut", TORIC, 5, (13,)), ("tiled", ROTATED, 13, (0, 0)), ("tiled", XZZX, 13, (0, 0)),
         ("tiled", PLANAR, 8, (0, 0))]
WHOLE = [(ROTATED, 5), (XZZX, 5), (PLANAR, 4), (TORIC, 3)]
SMALL = [(TORIC, 3), (XZZX, 3), (ROTATED, 3), (PLANAR, 3)]
# (code, L) -> the seed of its four pure-erasure shots at p_erase = 0.5: the first of 0, 1, ... whose reference has a shot with one non-zero class
# and a shot with several (test_pure_erasure_references_are_powers_of_two asserts it)
ERASURE_TOP = {(ROTATED, 21): 0, (PLANAR, 12): 1, (TORIC, 7): 0}

_top, _erasure = {}, {}


def qubit_cells(code, L):
    """bool[state shape]: the cells some generator acts on -- all but the planar array's idle row and column"""
    return (table(code, L)[0] != 0).any(axis=0).reshape(state_shape(code, L))


def factors_of(code, L, n, seed, p_erase=0.2):
    """(c, fx, fz, erased), each [n, state shape]: n rows of random factors (c in [0.5, 1], fx, fz log-uniform in [1e-2, 1]), a fraction p_erase of the
    qubits erased to c = fx = fz = 1; NaN in the cells that hold no qubit"""
    rng = np.random.default_rng([83, code, L, seed])
    cells = qubit_cells(code, L)
    erased = (rng.random((n,) + cells.shape) < p_erase) & cells
    c, fx, fz = US.random_factors(rng, (n,) + cells.shape, erased)
    for a in (c, fx, fz):
        a[:, ~cells] = np.nan
    return c, fx, fz, erased


def reference(code, L, chain, c, fx, fz):
    """the per-site sector product of every class with the chain's syndrome: float64[ncls]"""
    gens, parts, rank = table(code, L)
    return np.array([US.site_sector_product(gens, r, c, fx, fz, U.order_for(code, L), parts, rank) for r in class_chains(code, chain)])


def top_case(code, L):
    """one TOP shape's syndromes -- random_errors under seed [5, code, L] from its second chain on --, one table row per syndrome with a fifth of the
    qubits erased, and the references float64[n, ncls]: computed once and left unchanged (tests/test_gpu_class_sweep_site_sectors.py runs the same
    cases) -> dict(chains, wq [n, state shape, 4], erased, want)"""
    if (code, L) not in _top:
        n = {(c, l): k for c, l, k in TOP}[code, L]
        chains = random_errors(code, L, n + 1, np.random.default_rng([5, code, L]))[1:]
        c, fx, fz, erased = factors_of(code, L, n, seed=0)
        wq = US.site_table(c, fx, fz)
        want = np.stack([reference(code, L, chains[s], c[s], fx[s], fz[s]) for s in range(n)])
        for a in (chains, wq, erased, want):
            a.setflags(write=False)
        _top[code, L] = dict(chains=chains, wq=wq, erased=erased, want=want)
    return _top[code, L]


def erasure_top_case(code, L, n=4):
    """n shots of the pure-erasure channel at p_erase = 0.5, computed once and left unchanged: dict(erased, errors: uniform Paulis on the erased
    qubits -- they are the chains --, wq: (1, 0, 0, 0) off the set and (1, 1, 1, 1) on it, eq_true, want float64[n, ncls]: the product under
    c = 1 and fx = fz = the set's indicator)"""
    if (code, L) not in _erasure:
        rng = np.random.default_rng([89, code, L, ERASURE_TOP[code, L]])
        cells = qubit_cells(code, L)
        erased = (rng.random((n,) + cells.shape) < 0.5) & cells
        errors = np.zeros(erased.shape, np.uint8)
        errors[erased] = rng.integers(0, 4, size=int(erased.sum()), dtype=np.uint8)
        wq = np.zeros(erased.shape + (4,))
        wq[..., 0] = 1.0
        wq[erased] = 1.0
        f = erased.astype(np.float64)
        want = np.stack([reference(code, L, errors[s], np.ones(cells.shape), f[s], f[s]) for s in range(n)])
        eq_true = classes(code, errors)
        for a in (erased, errors, wq, want, eq_true):
            a.setflags(write=False)
        _erasure[code, L] = dict(erased=erased, errors=errors, wq=wq, want=want, eq_true=eq_true)
    return _erasure[code, L]


def general_tables(code, L, n, seed=0):
    """n tables that do not factorise -- w_I uniform in [0.5, 1], w_X, w_Y, w_Z log-uniform in [1e-2, 1], each on its own: no sector law holds --,
    NaN in the cells that hold no qubit: float64[n, state shape, 4].  (util_site.random_site_weights goes down to 1e-3 on all four, which may
    underflow over the 441 qubits of L = 21.)"""
    rng = np.random.default_rng([97, code, L, seed])
    cells = qubit_cells(code, L)
    wq = np.exp(rng.uniform(np.log(1e-2), 0.0, size=(n,) + cells.shape + (4,)))
    wq[..., 0] = rng.uniform(0.5, 1.0, size=(n,) + cells.shape)
    wq[:, ~cells] = np.nan
    return wq


def assert_high_fixed_close(T, code, L, width, tile_width=0):
    """the plan of the shape closes a pair on a fixed slot >= 16, outside its segment's tile"""
    high = closes_on_high_fixed_slots(T, code, L, tile_width)
    print("%s L=%d tile_width %d: %d CLOSE pairs on fixed slots >= 16, slots %s" % (NAME[code], L, tile_width, len(high), sorted({s for _, s in high})))
    assert high and all(16 <= s < width for _, s in high) and tiled.info(T, code, L, 0, tile_width)[1]["width"] == width
    return high


@pytest.fixture(scope="module")
def T():
    return site.load_twin()


# ------------------------------------------------------------------------------------------------------ 1. a brute force over the group
@pytest.mark.parametrize("code,L", SMALL)
def test_the_site_product_is_a_brute_force_over_the_group_at_L3(code, L):
    """every class of two syndromes, a table row of its own each: the sum over all 2^G subsets of the oracle's generators of the product over the
    qubits of the table's entry, over 2^(G - rank)"""
    gens, _, rank = table(code, L)
    grp, used = span(gens), (gens != 0).any(axis=0)
    c, fx, fz, erased = factors_of(code, L, 2, seed=1, p_erase=0.3)
    wq = US.site_table(c, fx, fz).reshape(2, -1, 4)
    assert erased.any() and not erased.all() and np.isnan(wq[:, ~used]).all() and np.all(wq[:, used] > 0)
    for s, m in enumerate(random_errors(code, L, 3, np.random.default_rng([4, code, L]))[1:]):
        want = np.array([wq[s][np.flatnonzero(used), (grp ^ r)[:, used]].prod(axis=-1).sum() for r in class_chains(code, m)]) / 2.0 ** (len(gens) - rank)
        got = reference(code, L, m, c[s], fx[s], fz[s])
        print(NAME[code], L, "max relative difference %.3g" % S.rel(got, want).max())
        assert S.rel(got, want).max() < 1e-12 and np.all(want > 0)


def test_zero_factors_are_legal_and_a_free_bit_is_its_qubits_factor():
    """fx = 0 on a qubit kills exactly the chains with an x bit there -- against the brute force.  No code here has a bit of a used qubit that no
    generator owns, so the free-bit factor is exercised on a cut-down table: one sector and a single generator of the other"""
    gens, _, rank = table(ROTATED, 3)
    grp = span(gens)
    c, fx, fz, _ = factors_of(ROTATED, 3, 1, seed=2, p_erase=0.0)
    c, fx, fz = c[0].ravel(), fx[0].ravel(), fz[0].ravel()
    fx[[0, 4]], fz[7] = 0.0, 0.0
    wq = US.site_table(c, fx, fz)
    shaped = random_errors(ROTATED, 3, 3, np.random.default_rng(9))[2]
    m = shaped.ravel()
    for r in class_chains(ROTATED, shaped):
        want = wq[np.arange(9), grp ^ r].prod(axis=-1).sum()
        got = US.site_sector_product(gens, r, c, fx, fz)
        assert abs(got - want) <= 1e-12 * want and want > 0
    # drop the generators of one sector but one: the bits they owned alone become free, and the product still equals the brute force over what is left
    parts = U.sectors(gens)
    keep = np.sort(np.concatenate([parts[0][0], parts[1][0][:1]]))
    sub, fx2 = gens[keep], np.where(fx == 0.0, 0.3, fx)
    wq2 = US.site_table(c, fx2, fz)
    used, sub_grp = (sub != 0).any(axis=0), span(sub)
    chain = np.where(used, m, 0).astype(np.uint8)
    have, own = U.bit_rows(chain), U.bit_rows(sub).any(axis=0)
    assert (have & ~own).any()                                                  # the case has a set bit that nothing owns
    want = wq2[np.flatnonzero(used), (sub_grp ^ chain)[:, used]].prod(axis=-1).sum() / 2.0 ** (len(sub) - U.gf2_rank(U.bit_rows(sub)))
    assert abs(US.site_sector_product(sub, chain, c, fx2, fz) - want) <= 1e-12 * want and want > 0


# ------------------------------------------------------------------------------------------------------ 2. the whole lattice
@pytest.mark.parametrize("code,L", WHOLE)
def test_the_site_product_is_the_elimination_on_the_whole_lattice(code, L):
    gens, _, rank = table(code, L)
    c, fx, fz, erased = factors_of(code, L, 2, seed=3)
    wq = US.site_table(c, fx, fz).reshape(2, -1, 4)
    assert erased.any()
    for s, m in enumerate(random_errors(code, L, 3, np.random.default_rng([6, code, L]))[1:]):
        want = np.array([eliminate_site(gens, r, wq[s], U.order_for(code, L)) for r in class_chains(code, m)]) / 2.0 ** (len(gens) - rank)
        got = reference(code, L, m, c[s], fx[s], fz[s])
        print(NAME[code], L, "max relative difference %.3g" % S.rel(got, want).max())
        assert S.rel(got, want).max() < 1e-12 and np.all(want > 0)


# ------------------------------------------------------------------------------------------------------ 3. the site twins, all three routes
@pytest.mark.parametrize("route,code,L,widths", TWINS)
def test_the_site_product_is_the_site_twins(T, route, code, L, widths):
    """two syndromes under one table, then under a table each (NaN in the planar array's idle cells both times)"""
    chains = random_errors(code, L, 3, np.random.default_rng([5, code, L]))[1:]
    c, fx, fz, erased = factors_of(code, L, 2, seed=4)
    wq = US.site_table(c, fx, fz)
    assert erased.any()
    for rows in (1, 2):
        z, cls = site.twin(T, route, code, L, chains, wq if rows == 2 else wq[0], widths)
        assert np.array_equal(cls, classes(code, chains))
        want = np.stack([reference(code, L, m, *(a[s if rows == 2 else 0] for a in (c, fx, fz))) for s, m in enumerate(chains)])
        print("%s %s L=%d, %d table(s): max relative difference %.3g" % (route, NAME[code], L, rows, S.rel(z, want).max()))
        assert S.rel(z, want).max() < 1e-12 and np.all(want > 0) and len({r.tobytes() for r in want}) == 2


# ------------------------------------------------------------------------------------------------------ 4. the tiled twin above L = 13
@pytest.mark.parametrize("code,L,width", HIGH)
def test_the_site_product_is_the_site_tiled_twin_where_a_fixed_slot_is_16_or_above(T, code, L, width):
    assert_high_fixed_close(T, code, L, width)
    m = random_errors(code, L, 2, np.random.default_rng([5, code, L]))[1:]
    c, fx, fz, erased = factors_of(code, L, 1, seed=5)
    z, cls = site.twin(T, "tiled", code, L, m, US.site_table(c, fx, fz), (0, 0))
    want = reference(code, L, m[0], c[0], fx[0], fz[0])
    gap = min(abs(a - b) / max(a, b) for i, a in enumerate(want) for b in want[:i])
    print("%s L=%d: max relative difference %.3g, closest pair of classes %.3g apart" % (NAME[code], L, S.rel(z[0], want).max(), gap))
    assert S.rel(z[0], want).max() < 1e-12 and np.all(want > 1e-200) and gap > 1e-6 and np.array_equal(cls, classes(code, m))


# ------------------------------------------------------------------------------------------------------ 5. the cases of the GPU test
@pytest.mark.parametrize("code,L,n", TOP)
def test_top_references_are_finite_and_tell_classes_and_syndromes_apart(code, L, n):
    """the reference runs within eliminate_site's 16 open generators (its own assertion); every Z is finite and far above the underflow; no two classes
    of a syndrome are closer than 1e-6 relative, so a class written to another's column shows at the GPU test's 1e-10; the rows differ, so a
    syndrome that read another's table shows"""
    case = top_case(code, L)
    want, wq, cells = case["want"], case["wq"], qubit_cells(code, L)
    assert want.shape == (n, 16 if code == TORIC else 4) and np.all(np.isfinite(want)) and np.all(want > 1e-200)
    assert np.all(wq[:, cells] > 0) and np.isnan(wq[:, ~cells]).all() and np.all(wq[case["erased"]] == 1.0)
    share = case["erased"][:, cells].mean()
    assert 0.15 < share < 0.25 and len({t.tobytes() for t in wq}) == n
    for row in want:
        gap = min(abs(a - b) / max(a, b) for i, a in enumerate(row) for b in row[:i])
        print("%s L=%d: class weights %.6g .. %.6g, closest pair %.3g apart" % (NAME[code], L, row.min(), row.max(), gap))
        assert gap > 1e-6
    assert len({r.tobytes() for r in want}) == n
    for i in range(n):                                                          # (no entry of another row could pass for this one's)
        for j in range(i):
            assert np.all(np.abs(want[i] - want[j]) > 1e-3 * np.maximum(want[i], want[j]))


def check_power_of_two_law(z, eq_true):
    """every entry 0 or a power of two, the true class never 0 -> (shots with one non-zero class, shots with several)"""
    one = several = 0
    for s, row in enumerate(z):
        live = row[row != 0.0]
        assert len(live) >= 1 and np.all(np.frexp(live)[0] == 0.5) and np.all(live == live[0]), (s, row)
        assert row[eq_true[s]] != 0.0, (s, row)
        one, several = one + (len(live) == 1), several + (len(live) > 1)
    return one, several


@pytest.mark.parametrize("code,L", sorted(ERASURE_TOP))
def test_pure_erasure_references_are_powers_of_two(code, L):
    case = erasure_top_case(code, L)
    one, several = check_power_of_two_law(case["want"], case["eq_true"])
    print("%s L=%d: shots with one non-zero class %d, with several %d, largest 2^%d" % (NAME[code], L, one, several, int(np.log2(case["want"].max()))))
    assert one >= 1 and several >= 1 and case["want"].max() >= 4.0
