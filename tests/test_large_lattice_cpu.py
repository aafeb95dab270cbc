"""The host twins of the lift and the corrections at the top of the accepted range, without a GPU: what test_syndrome_lift_cpu.py and
test_corrections_cpu.py pin at L <= 7 / 21, at the shapes on either side of the 64 KiB LDS window and at L = 63 / 64 (util_large_lattice.BRANCH)
-- the references tests/test_gpu_large_lattice.py compares the kernels with.

Every comparison is exact.  The local-minimum check takes the energy change of every generator from its four sites instead of a dense
[N, n_gen, nq] array; the corrections run on 5 errors x 16 targets (toric) or 18 x 4 (the others) with three candidates a row."""
import ctypes as C

import numpy as np
import pytest

import test_corrections_cpu as corr_cpu
import test_syndrome_lift_cpu as lift_cpu
import util_large_lattice as U
from oracle import oracle as orc
from qecmc import _lib as L_
from test_syndrome_lift_cpu import PLANAR, TORIC, n_cells, oracle_syndrome, state_shape

_u8p, _u32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def T():
    return corr_cpu.load_twin()


@pytest.mark.parametrize("code,L", U.LIFT_SHAPES + [(TORIC, 47)], ids=U.ids(U.LIFT_SHAPES + [(TORIC, 47)]))
def test_shapes_sit_on_their_branch(T, code, L):
    assert U.on_branch(T, code, L) == (L >= 46 and code in (TORIC, PLANAR))
    assert U.BRANCH[code, L][1] <= 131072                             # what the launchers ask the runtime for, once


@pytest.mark.parametrize("code,L", U.LIFT_SHAPES, ids=U.ids(U.LIFT_SHAPES))
def test_table_rows_have_their_own_check_as_syndrome(T, code, L):
    """test_syndrome_lift_cpu's test of the same name, every qubit and every row (toric L = 64: 16 384 + 8 192 oracle calls), the rows unpacked one
    at a time"""
    nq, cells = U.nq_of(code, L), n_cells(code, L)
    W = U.BRANCH[code, L][0]
    buf = np.zeros(cells * (W + 1), dtype=np.uint32)
    assert T.qt_lift_table(code, L, buf.ctypes.data_as(_u32p), buf.size) == buf.size
    t = buf.reshape(cells, W + 1)
    flags = t[:, W]
    hit = np.zeros(cells, dtype=bool)
    m = np.zeros(state_shape(code, L), dtype=np.uint8)
    for q in range(nq):
        if code == PLANAR and q >= L * L and ((q - L * L) // L == L - 1 or (q - L * L) % L == L - 1):
            continue                                                  # (an idle cell of the planar layout holds no qubit)
        for P in (1, 3):
            m.flat[q] = P
            s = oracle_syndrome(code, m)
            assert 1 <= s.sum() <= 2
            hit |= s.astype(bool)
        m.flat[q] = 0
    assert np.array_equal(flags != 0, hit)
    assert not t[flags == 0].any()
    q = np.arange(nq)
    word, shift = q >> 4, ((q & 15) * 2).astype(np.uint32)
    roots = {}
    for cell in np.flatnonzero(flags):
        chain = ((t[cell, word] >> shift) & 3).astype(np.uint8)
        s = oracle_syndrome(code, chain.reshape(state_shape(code, L)))
        s[cell] ^= 1
        if code == TORIC:
            assert s.sum() == 1, cell
            roots.setdefault(int(flags[cell]), set()).add(int(np.flatnonzero(s)[0]))
        else:
            assert not s.any(), cell
            assert flags[cell] == 1
    if code == TORIC:
        assert roots == {3: {0}, 5: {L * L}}


@pytest.mark.parametrize("code,L", U.LIFT_SHAPES, ids=U.ids(U.LIFT_SHAPES))
def test_lifted_chains(T, code, L):
    c = U.lift_case(code, L)
    d, bad = c["defects"], c["bad"]
    good = np.setdiff1d(np.arange(U.N), bad)
    assert len(bad) == (0 if code == PLANAR else 2)
    (plain, st0, w0), (low, st1, w1) = c["plain"], c["low"]
    # conditions on the reference alone: the lift finds something, and the descent has something to do
    assert w0[good].max() > 0 and (w1[good] < w0[good]).any() and not np.array_equal(plain, low)
    for chains, st, w in ((plain, st0, w0), (low, st1, w1)):
        assert np.array_equal(np.flatnonzero(st), bad) and set(st.tolist()) <= {0, 1}
        assert np.array_equal(np.stack([oracle_syndrome(code, x) for x in chains[good]]), d[good])
        assert np.array_equal(w[good], [orc.count_errors(x) for x in chains[good]])
        assert not chains[bad].any() and np.all(w[bad] == -1)         # no syndrome of the code: status 1, weight -1, the zero chain
    assert np.all(w1 <= w0)
    assert not plain[0].any() and not low[0].any()                    # the zero syndrome gives the zero chain
    assert U.generator_changes(code, L, low).min() >= 0               # after the descent no generator lowers the error count
    assert U.generator_changes(code, L, plain[good]).min() < 0        # (... and the check can see one that does)


@pytest.mark.parametrize("L", [46, 64])
def test_toric_even_sizes_have_no_class_move(T, L):
    buf = np.zeros(256, dtype=np.uint32)
    assert T.qt_class_moves(TORIC, L, buf.ctypes.data_as(_u32p), buf.size) == 0
    nq = 2 * L * L
    cand, tgt, out = np.zeros((1, nq), np.uint8), np.zeros(1, np.int32), np.zeros((1, nq), np.uint8)
    assert T.qt_corrections(TORIC, L, 1, 1, cand.ctypes.data_as(_u8p), tgt.ctypes.data_as(_i32p), 1, 1, out.ctypes.data_as(_u8p), None, None, None, None) == -4
    lib = L_.lib()
    assert lib.qecmc_corrections(TORIC, L, 1, 1, L_.u8(cand), L_.i32(tgt), 1, 1, L_.u8(out), None, None, None, None) == -4
    msg = lib.qecmc_last_error()
    assert b"L=%d" % L in msg and b"even length" in msg
    cr = C.c_void_p()
    assert lib.qecmc_corrector_create(TORIC, L, C.byref(cr)) == -4 and not cr.value


@pytest.mark.parametrize("code,L", U.CORRECTION_SHAPES, ids=U.ids(U.CORRECTION_SHAPES))
def test_class_move_table(T, code, L):
    need = corr_cpu.class_moves(T, code, L)
    kinds = 4 if code == TORIC else 2
    assert need.max() < (1 << kinds) and not np.diag(need).any()
    chains = lift_cpu.random_errors(code, L, 6, np.random.default_rng([11, code, L]))
    seen = set()
    for m in chains:
        a = corr_cpu.oracle_class(code, m)
        seen.add(a)
        for b in range(corr_cpu.ncls_of(code)):
            moved = m
            for kind in range(kinds):
                if need[a, b] >> kind & 1:
                    moved = corr_cpu.apply_kind(code, moved, kind)
            assert corr_cpu.oracle_class(code, moved) == b, (a, b, need[a, b])
            assert np.array_equal(oracle_syndrome(code, moved), oracle_syndrome(code, m))
    assert len(seen) > 1


@pytest.mark.parametrize("code,L", U.CORRECTION_SHAPES, ids=U.ids(U.CORRECTION_SHAPES))
def test_corrections(T, code, L):
    """test_corrections_cpu's test_properties and the pick rule of its test_three_candidates, the four (place, descend) settings in one pass"""
    c = U.correction_case(code, L)
    cand, target = c["cand"], c["target"]
    inside = c["cand_class"] == target[:, None]
    some = inside.any(axis=1)
    wk = c["cand_weight"]
    want_source = np.where(some, np.argmin(np.where(inside, wk, 1 << 30), axis=1), np.argmin(wk, axis=1))   # (argmin: the first of equals)
    # conditions on the reference alone
    assert some.any() and (~some).any()                               # some rows are moved and some are not
    assert len(set(want_source.tolist())) >= 2                        # at least two different sources
    zero_class = corr_cpu.oracle_class(code, np.zeros(state_shape(code, L), np.uint8))
    got = {s: corr_cpu.twin(T, code, L, cand, target, *s) for s in corr_cpu.SETTINGS}
    for place in (0, 1):
        assert not np.array_equal(got[place, 0]["corrections"], got[place, 1]["corrections"])              # the descent changes at least one row
    for (place, descend), g in got.items():
        cor = g["corrections"]
        assert not g["status"].any()
        assert np.array_equal(g["source"], want_source) and np.array_equal(g["moved"], ~some)
        assert np.array_equal(corr_cpu.syndromes(code, cor), c["defects"])
        assert np.array_equal(corr_cpu.classes(code, cor), target)
        assert np.array_equal(g["weight"], corr_cpu.weights(cor))
        if descend:
            assert U.generator_changes(code, L, cor).min() >= 0       # a local minimum: no generator lowers the weight
        else:
            keep = np.flatnonzero(some)
            assert np.array_equal(cor[keep], cand[keep, want_source[keep]])                                 # nothing to do: the candidate itself
        # error ^ correction is a stabilizer iff the target is the error's class -- on every row, exactly
        residual = c["errors"] ^ cor
        stabilizer = ~corr_cpu.syndromes(code, residual).any(axis=1) & (corr_cpu.classes(code, residual) == zero_class)
        assert np.array_equal(stabilizer, target == c["err_class"])
