"""The sector product of tests/util_sectors.py, without a GPU: pinned here before tests/test_gpu_class_sweep_sectors.py lets it judge the tiled
sweep at the shapes no host twin reaches (rotated / xzzx L = 21, planar L = 12, toric L = 7).

What is pinned: every code's generator table falls into exactly two sectors at every shape used; the product equals a brute force over the whole
group (test_enumerate_cpu.span) at L = 3 for every class; it equals the host twins -- the tiled twin, and the LDS sweep's where the shape is its --
over all classes of three syndromes each up to rotated / xzzx L = 13, planar L = 8 and toric L = 5; at the shapes the GPU tests use, the class
weights of one syndrome are positive and pairwise different, so a permuted class would show; the top shapes stay within eliminate's 16 axes.

Tolerance 1e-12 relative per class weight, as tests/test_class_sweep_tiled_cpu.py: either side is a sum of positive terms and errs by about
(nq + G) 2^-53 -- 1e-13 at L = 21.  Measured: at most 2e-15."""
import numpy as np
import pytest

import test_class_sweep_cpu as S
import test_class_sweep_tiled_cpu as tiled
import util_sectors as U
from test_corrections_cpu import classes, generators
from test_enumerate_cpu import class_chains, span
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors

NAME = S.NAME
FX, FZ = 0.15 / 0.85, 0.075 / 0.85
WP = np.array([1.0, FX, FX * FZ, FZ])                                           # w_Y = w_X w_Z, w_X != w_Z
# (code, L, syndromes): where tests/test_gpu_class_sweep_sectors.py holds the tiled sweep against the product
TOP = [(ROTATED, 21, 2), (XZZX, 21, 2), (PLANAR, 12, 2), (TORIC, 7, 1), (PLANAR, 10, 2), (XZZX, 17, 2)]
# (code, L, hbm_width of the tiled twin): where a host twin is cheap; toric L = 5 with the cut plan's 8 held generators
TWINS = [(XZZX, 5, 0), (XZZX, 9, 0), (XZZX, 13, 0), (ROTATED, 9, 0), (ROTATED, 13, 0), (PLANAR, 4, 0), (PLANAR, 8, 0), (TORIC, 3, 0), (TORIC, 5, 13)]
SMALL = [(TORIC, 3), (XZZX, 3), (ROTATED, 3), (PLANAR, 3)]

_tables, _top = {}, {}


def table(code, L):
    """(the oracle's stencils, their sectors, their rank), computed once per shape"""
    if (code, L) not in _tables:
        gens = generators(code, L)
        _tables[code, L] = (gens, U.sectors(gens), U.gf2_rank(U.bit_rows(gens)))
    return _tables[code, L]


def reference(code, L, chain):
    """the sector product of every class with the chain's syndrome: float64[ncls]"""
    gens, parts, rank = table(code, L)
    return np.array([U.sector_product(gens, r, FX, FZ, U.order_for(code, L), parts, rank) for r in class_chains(code, chain)])


def top_case(code, L):
    """the syndromes of one TOP shape -- random_errors under seed [5, code, L] from its second chain on (site probability 0.15, then 0.4) -- and their
    references float64[n, ncls], computed once and left unchanged (tests/test_gpu_class_sweep_sectors.py runs the same cases)"""
    if (code, L) not in _top:
        n = {(c, l): k for c, l, k in TOP}[code, L]
        chains = random_errors(code, L, 3, np.random.default_rng([5, code, L]))[1:1 + n]
        want = np.stack([reference(code, L, m) for m in chains])
        for a in (chains, want):
            a.setflags(write=False)
        _top[code, L] = (chains, want)
    return _top[code, L]


@pytest.fixture(scope="module")
def T():
    return tiled.load_twin()


@pytest.mark.parametrize("code,L", sorted(set(SMALL) | {(c, L) for c, L, _ in TOP + TWINS} | {(ROTATED, 15), (XZZX, 15), (ROTATED, 17)}))
def test_every_table_falls_into_two_sectors(code, L):
    gens, parts, rank = table(code, L)
    assert len(parts) == 2 and rank == (len(gens) - 2 if code == TORIC else len(gens))
    sizes = sorted(len(idx) for idx, _ in parts)
    print("%s L=%d: sectors of %d and %d generators, rank %d" % (NAME[code], L, sizes[0], sizes[1], rank))
    assert sum(sizes) == len(gens) and sizes[0] >= len(gens) // 2 - L
    if code == TORIC:                                                           # the vertex generators and the plaquette generators
        assert all(len(set(np.unique(gens[idx]).tolist()) - {0}) == 1 for idx, _ in parts)
    if code == XZZX and L > 3:                                                  # two checkerboards, X and Z mixed in either
        assert all(set(np.unique(gens[idx]).tolist()) == {0, 1, 3} for idx, _ in parts)


def test_the_rank_of_this_file_is_a_rank():
    rng = np.random.default_rng(12)
    rows = rng.integers(0, 2, size=(9, 14)).astype(bool)
    dep = np.stack([rows[0] ^ rows[3], rows[1] ^ rows[2] ^ rows[8], rows[5]])
    assert U.gf2_rank(rows) == 9 and U.gf2_rank(np.concatenate([rows, dep])) == 9 and U.gf2_rank(np.zeros((3, 5), bool)) == 0
    assert U.gf2_rank(np.eye(6, dtype=bool)[[0, 2, 2, 5]]) == 3


@pytest.mark.parametrize("code,L", SMALL)
def test_the_product_is_a_brute_force_over_the_group_at_L3(code, L):
    """every class of two syndromes: sum over all 2^G subsets of the oracle's generators of the product of the weights, over 2^(G - rank)"""
    gens, _, rank = table(code, L)
    grp = span(gens)
    assert len(grp) == 1 << len(gens)
    for m in random_errors(code, L, 3, np.random.default_rng([4, code, L]))[1:]:
        reps = class_chains(code, m)
        want = np.array([WP[grp ^ r].prod(axis=-1).sum() for r in reps]) / 2.0 ** (len(gens) - rank)
        got = reference(code, L, m)
        print(NAME[code], L, "max relative difference %.3g" % S.rel(got, want).max())
        assert S.rel(got, want).max() < 1e-12 and np.all(want > 0)


def test_a_chain_bit_no_generator_owns_is_a_plain_factor():
    """the planar code's idle row and column: qubits of the array no generator acts on"""
    gens, parts, rank = table(PLANAR, 3)
    idle = np.flatnonzero(~(gens != 0).any(axis=0))
    assert len(idle) == 5
    m = random_errors(PLANAR, 3, 2, np.random.default_rng(9))[1].ravel()
    base = U.sector_product(gens, m, FX, FZ, U.order_for(PLANAR, 3))
    for pauli, f in ((1, FX), (2, FX * FZ), (3, FZ)):
        moved = m.copy()
        moved[idle[1]] = pauli
        assert abs(U.sector_product(gens, moved, FX, FZ, U.order_for(PLANAR, 3)) / (base * f) - 1) < 1e-14


@pytest.mark.parametrize("code,L,hbm_width", TWINS)
def test_the_product_is_the_host_twins(T, code, L, hbm_width):
    chains = random_errors(code, L, 3, np.random.default_rng([5, code, L]))
    z, cls = tiled.twin(T, code, L, chains, WP, hbm_width)
    assert np.array_equal(cls, classes(code, chains)) and tiled.info(T, code, L, hbm_width)[1]["held"] == (8 if hbm_width else 0)
    want = np.stack([reference(code, L, m) for m in chains])
    print(NAME[code], L, "tiled twin: max relative difference %.3g" % S.rel(z, want).max())
    assert S.rel(z, want).max() < 1e-12 and np.all(want > 0)
    if S.info(T, code, L)[0] == 0:                                              # a shape of the LDS sweep: its twin too
        z, _ = S.twin(T, code, L, chains, WP)
        print(NAME[code], L, "sweep twin: max relative difference %.3g" % S.rel(z, want).max())
        assert S.rel(z, want).max() < 1e-12


@pytest.mark.parametrize("code,L,n", TOP)
def test_top_shapes_complete_and_their_classes_can_be_told_apart(code, L, n):
    """the reference runs within eliminate's 16 open generators (its own assertion), and no two classes of a syndrome are closer than 1e-6 relative:
    a class written to another's column would show at the GPU test's 1e-10"""
    chains, want = top_case(code, L)
    assert want.shape == (n, 16 if code == TORIC else 4) and np.all(want > 0) and np.all(np.isfinite(want))
    for row in want:
        gap = min(abs(a - b) / max(a, b) for i, a in enumerate(row) for b in row[:i])
        print("%s L=%d: class weights %.6g .. %.6g, closest pair %.3g apart" % (NAME[code], L, row.min(), row.max(), gap))
        assert gap > 1e-6
    assert len({r.tobytes() for r in want}) == n
