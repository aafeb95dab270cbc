"""Start chains from bare syndromes, without a GPU: the lift table of csrc/syndrome_lift.hpp and the lift-and-descend body the kernel runs,
compiled by g++ into the host-table test library (qt_lift_table, qt_chains_from_syndromes), against the oracle's syndrome functions and stencils.

What is pinned: every table row's syndrome is its own check (on the torus: plus the root of its component); a lifted chain reproduces the
defects it came from, with and without the greedy descent; the descent ends in a local minimum of the weight (no generator lowers it); and --
because the lifted chain has the error's syndrome -- the exact class law computed from it is the law computed from the error itself.  No
class-law test of a finite run from a lifted start: the lift lands in an arbitrary class and only the burn-in depends on it."""
import ctypes as C

import numpy as np
import pytest

from hostlib import PLANAR, ROTATED, TORIC, XZZX, run_selftest, tables_lib
from oracle import oracle as orc
from qecmc import _lib as L_
from util_exact import toric_class_probabilities

ORC_CODE = {TORIC: orc.TORIC, XZZX: orc.XZZX, ROTATED: orc.ROTATED, PLANAR: orc.PLANAR}
SHAPES = [(c, L) for c in (TORIC, XZZX, ROTATED, PLANAR) for L in (3, 5, 7)] + [(TORIC, 4), (TORIC, 15), (ROTATED, 21)]
_u8p, _u32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


def load_twin():
    """the host-table test library with the lift's two entry points (tests/test_gpu_syndrome_lift.py compares the GPU with it)"""
    lib = tables_lib()
    lib.qt_lift_table.restype = C.c_int
    lib.qt_lift_table.argtypes = [C.c_int, C.c_int, _u32p, C.c_int]
    lib.qt_chains_from_syndromes.restype = C.c_int
    lib.qt_chains_from_syndromes.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, C.c_int, _u8p, _u8p, _i32p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def state_shape(code, L):
    return (2, L, L) if code in (TORIC, PLANAR) else (L, L)


def n_cells(code, L):
    return 2 * L * L if code == TORIC else 2 * L * (L - 1) if code == PLANAR else (L + 1) * (L + 1)


def oracle_syndrome(code, m):
    """the oracle's defects of one configuration in the flat layout qecmc_syndrome writes"""
    if code == TORIC:
        return orc.toric_syndrome(m).ravel().astype(np.uint8)
    if code == PLANAR:
        v, q = orc.planar_syndrome(m)
        return np.concatenate([v.ravel(), q.ravel()]).astype(np.uint8)
    return orc.surf_syndrome(ORC_CODE[code], m).ravel().astype(np.uint8)


def random_errors(code, L, n, rng):
    """n random errors, site probabilities 0.05 / 0.15 / 0.4 in turn, the planar idle row and column kept zero"""
    m = np.zeros((n,) + state_shape(code, L), dtype=np.uint8)
    p = np.array([0.05, 0.15, 0.4])[np.arange(n) % 3].reshape((n,) + (1,) * (m.ndim - 1))
    err = rng.random(m.shape) < p
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    if code == PLANAR:
        m[:, 1, -1, :] = 0
        m[:, 1, :, -1] = 0
    return m


def lift_table(T, code, L):
    """(rows as uint8 chains [cells, nq], flags uint32[cells])"""
    nq = int(np.prod(state_shape(code, L)))
    W = (nq + 15) // 16
    buf = np.zeros(n_cells(code, L) * (W + 1), dtype=np.uint32)
    n = T.qt_lift_table(code, L, buf.ctypes.data_as(_u32p), buf.size)
    assert n == buf.size
    t = buf.reshape(n_cells(code, L), W + 1)
    q = np.arange(nq)
    chains = ((t[:, q >> 4] >> ((q & 15) * 2).astype(np.uint32)) & 3).astype(np.uint8)
    return chains, t[:, W].copy()


def twin(T, code, L, defects, descend):
    d = np.ascontiguousarray(defects, dtype=np.uint8)
    n, nq = d.shape[0], int(np.prod(state_shape(code, L)))
    chains, status, weight = np.full((n, nq), 9, np.uint8), np.full(n, 9, np.uint8), np.full(n, 9, np.int32)
    rc = T.qt_chains_from_syndromes(code, L, n, d.ctypes.data_as(_u8p), int(descend), chains.ctypes.data_as(_u8p), status.ctypes.data_as(_u8p),
                                    weight.ctypes.data_as(_i32p))
    assert rc == 0
    return chains.reshape((n,) + state_shape(code, L)), status, weight


def batch(code, L, n=200, seed=0):
    """n random errors of a shape and their oracle syndromes (row 0: no error)"""
    m = random_errors(code, L, n, np.random.default_rng([seed, code, L]))
    m[0] = 0
    return m, np.stack([oracle_syndrome(code, x) for x in m])


@pytest.mark.parametrize("code,L", SHAPES)
def test_table_rows_have_their_own_check_as_syndrome(T, code, L):
    chains, flags = lift_table(T, code, L)
    cells = n_cells(code, L)
    # the cells some single-qubit X or Z sets: exactly the cells with a row; and no single-qubit error sets more than two
    hit = np.zeros(cells, dtype=bool)
    zero = np.zeros(state_shape(code, L), dtype=np.uint8)
    for q in range(zero.size):
        if code == PLANAR and q >= L * L and ((q - L * L) // L == L - 1 or (q - L * L) % L == L - 1):
            continue                                                       # (an idle cell of the planar layout holds no qubit)
        for P in (1, 3):
            m = zero.copy()
            m.flat[q] = P
            s = oracle_syndrome(code, m)
            assert 1 <= s.sum() <= 2
            hit |= s.astype(bool)
    assert np.array_equal(flags != 0, hit)
    assert not chains[flags == 0].any()
    # every row's syndrome: its own cell, on the torus plus the root of its component (the lowest cell of the component)
    roots = {}
    for cell in np.flatnonzero(flags):
        s = oracle_syndrome(code, chains[cell].reshape(state_shape(code, L)))
        s[cell] ^= 1
        if code == TORIC:
            assert s.sum() == 1, cell
            roots.setdefault(int(flags[cell]), set()).add(int(np.flatnonzero(s)[0]))
        else:
            assert not s.any(), cell
            assert flags[cell] == 1                                        # one component, through the boundary node: no parity to keep
    if code == TORIC:
        assert sorted(roots) == [3, 5]                                     # two components without boundary
        assert roots == {3: {0}, 5: {L * L}}


@pytest.mark.parametrize("code,L", SHAPES)
def test_round_trip_and_local_minimum(T, code, L):
    errors, defects = batch(code, L)
    plain, st0, w0 = twin(T, code, L, defects, 0)
    low, st1, w1 = twin(T, code, L, defects, 1)
    assert not st0.any() and not st1.any()
    for chains, w in ((plain, w0), (low, w1)):
        assert np.array_equal(np.stack([oracle_syndrome(code, c) for c in chains]), defects)
        assert np.array_equal(w, [orc.count_errors(c) for c in chains])
    assert np.all(w1 <= w0)
    assert not plain[0].any() and not low[0].any() and w0[0] == 0 and w1[0] == 0          # the zero syndrome gives the zero chain
    # after the descent no generator lowers the error count
    if code == TORIC:
        gens = [(r, c, op) for op in (1, 3) for r in range(L) for c in range(L)]
        apply = orc.toric_apply_stabilizer
    else:
        gens = [orc.surf_gen_rco(ORC_CODE[code], L, g) for g in range(orc.surf_ngen(ORC_CODE[code], L))]
        apply = lambda m, r, c, op: orc.surf_apply_stabilizer(ORC_CODE[code], m, r, c, op)
    for c in low:
        assert min(apply(c, *g)[1] for g in gens) >= 0


@pytest.mark.parametrize("seed,p,Nc", [(1, 0.10, 3), (2, 0.15, 4), (3, 0.12, 4), (4, 0.20, 5)])
def test_same_syndrome_same_class_law(T, seed, p, Nc):
    """the inputs of test_gpu_stats.py::test_exact_enumeration_L3: the exact class law from the lifted chain is the law from the error"""
    rng = np.random.default_rng(seed)
    init = np.zeros((2, 3, 3), dtype=np.uint8)
    err = rng.random(init.shape) < 0.15
    init[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    P = toric_class_probabilities(init, p, orc.toric_apply_stabilizer, orc.toric_to_class)
    for descend in (0, 1):
        chain, status, _ = twin(T, TORIC, 3, oracle_syndrome(TORIC, init)[None], descend)
        assert status[0] == 0
        Q = toric_class_probabilities(chain[0], p, orc.toric_apply_stabilizer, orc.toric_to_class)
        assert np.max(np.abs(P - Q)) <= 1e-12


def test_refusals_leave_their_neighbours_alone(T):
    for code, L, bad_cell in ((TORIC, 5, 7), (XZZX, 5, 0)):               # one defect on the torus; cell (0, 0) of the xzzx grid is no check
        _, defects = batch(code, L, n=6, seed=1)
        good = twin(T, code, L, defects, 1)
        if code == TORIC:
            defects[2] = 0
        assert lift_table(T, code, L)[1][bad_cell] == (3 if code == TORIC else 0)
        defects[2, bad_cell] ^= 1
        chains, status, weight = twin(T, code, L, defects, 1)
        assert status.tolist() == [0, 0, 1, 0, 0, 0]
        assert not chains[2].any() and weight[2] == -1
        keep = [0, 1, 3, 4, 5]
        assert np.array_equal(chains[keep], good[0][keep]) and np.array_equal(weight[keep], good[2][keep])


def test_host_checks_need_no_device():
    lib = L_.lib()
    d, ch = np.zeros((1, 18), np.uint8), np.zeros((1, 18), np.uint8)
    lift = C.c_void_p()
    for call in (lambda: lib.qecmc_chains_from_syndromes(0, 3, 1, None, 1, L_.u8(ch), None, None),
                 lambda: lib.qecmc_chains_from_syndromes(0, 3, 1, L_.u8(d), 1, None, None, None),
                 lambda: lib.qecmc_lift_create(0, 3, None)):
        assert call() == -1 and b"NULL" in lib.qecmc_last_error()
    for code in (-1, 4):
        assert lib.qecmc_chains_from_syndromes(code, 3, 1, L_.u8(d), 1, L_.u8(ch), None, None) == -1 and b"code" in lib.qecmc_last_error()
        assert lib.qecmc_lift_create(code, 3, C.byref(lift)) == -1 and b"code" in lib.qecmc_last_error()
    assert lib.qecmc_chains_from_syndromes(1, 4, 1, L_.u8(d), 1, L_.u8(ch), None, None) == -1 and b"odd L" in lib.qecmc_last_error()
    assert lib.qecmc_lift_create(1, 4, C.byref(lift)) == -1 and b"odd L" in lib.qecmc_last_error()
    assert not lift.value


def test_lift_under_sanitizers():
    """a stand-alone program (its own main) built from syndrome_lift.hpp with -fsanitize=address,undefined: builds the tables, lifts random
    syndromes and refusals with and without the descent, checks every chain; run as a child process"""
    run_selftest("lift_asan", "syndrome_lift_selftest_asan")
