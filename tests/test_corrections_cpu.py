"""Corrections from decoded syndromes, without a GPU: the class-move table of csrc/corrections.hpp and the survey-pick-move-descend body the kernel
runs, compiled by g++ into the host-table test library (qt_class_moves, qt_corrections), against the oracle's syndrome, class and count functions and
its stencils.

What is pinned: need[a][b] takes any chain of class a to class b; a correction has the error's syndrome, lies in the target class, weighs what it
says, and -- after the descent -- is a local minimum of the weight; source and moved follow the pick rule; placing a logical operator never costs
more than position 0; and the identity the harness flag success_correction rests on: error ^ correction is a stabilizer iff target == class(error)."""
import ctypes as C

import numpy as np
import pytest

import test_syndrome_lift_cpu as lift_cpu
from hostlib import run_selftest
from oracle import oracle as orc
from qecmc import _lib as L_
from test_syndrome_lift_cpu import ORC_CODE, PLANAR, ROTATED, TORIC, XZZX, oracle_syndrome, state_shape

SHAPES = [(c, L) for c in (TORIC, XZZX, ROTATED, PLANAR) for L in (3, 5, 7)]
SETTINGS = [(0, 0), (0, 1), (1, 0), (1, 1)]                              # (place, descend)
N_ERR = 200
_u8p, _u32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
# kind k of the mask tables as the oracle's apply_logical operator: toric (op, layer); the others op (xzzx: 3 is Z; rotated / planar: 2 is Z)
TORIC_KINDS = [(1, 0), (3, 0), (1, 1), (3, 1)]
SURF_KINDS = {XZZX: (1, 3), ROTATED: (1, 2), PLANAR: (1, 2)}


def load_twin():
    """the host-table test library with the corrections' two entry points (tests/test_gpu_corrections.py compares the GPU with it)"""
    lib = lift_cpu.load_twin()
    lib.qt_class_moves.restype = C.c_int
    lib.qt_class_moves.argtypes = [C.c_int, C.c_int, _u32p, C.c_int]
    lib.qt_corrections.restype = C.c_int
    lib.qt_corrections.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint32, _u8p, _i32p, C.c_int, C.c_int, _u8p, _i32p, _i32p, _u8p, _u8p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def ncls_of(code):
    return 16 if code == TORIC else 4


def oracle_class(code, m):
    return orc.toric_eq_class(m) if code == TORIC else orc.surf_eq_class(ORC_CODE[code], m)


def classes(code, chains):
    return np.array([oracle_class(code, c) for c in chains], dtype=np.int32)


def weights(chains):
    return np.array([orc.count_errors(c) for c in chains], dtype=np.int32)


def syndromes(code, chains):
    return np.stack([oracle_syndrome(code, c) for c in chains])


def apply_kind(code, m, kind, pos=0):
    if code == TORIC:
        op, layer = TORIC_KINDS[kind]
        return orc.toric_apply_logical(m, op, layer, pos, pos)[0]
    return orc.surf_apply_logical(ORC_CODE[code], m, SURF_KINDS[code][kind], pos, pos)[0]


def generators(code, L):
    """every generator's Pauli pattern as a chain uint8[n_gen, nq]: the oracle's stencil on the zero chain"""
    zero = np.zeros(state_shape(code, L), dtype=np.uint8)
    if code == TORIC:
        return np.stack([orc.toric_apply_stabilizer(zero, r, c, op)[0].ravel() for op in (1, 3) for r in range(L) for c in range(L)])
    oc = ORC_CODE[code]
    return np.stack([orc.surf_apply_stabilizer(oc, zero, *orc.surf_gen_rco(oc, L, g))[0].ravel() for g in range(orc.surf_ngen(oc, L))])


def class_moves(T, code, L):
    n = ncls_of(code)
    buf = np.zeros(n * n, dtype=np.uint32)
    got = T.qt_class_moves(code, L, buf.ctypes.data_as(_u32p), buf.size)
    assert got == buf.size
    return buf.reshape(n, n)


def twin(T, code, L, candidates, target, place, descend):
    """the host twin on candidates [N, K, ...] -> dict of the five outputs (chains shaped like the code's state)"""
    shape = state_shape(code, L)
    nq = int(np.prod(shape))
    cand = np.ascontiguousarray(candidates, dtype=np.uint8).reshape(len(candidates), -1, nq)
    n, k = cand.shape[:2]
    tgt = np.ascontiguousarray(target, dtype=np.int32)
    out, weight, source = np.full((n, nq), 9, np.uint8), np.full(n, 9, np.int32), np.full(n, 9, np.int32)
    moved, status = np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)
    rc = T.qt_corrections(code, L, n, k, cand.ctypes.data_as(_u8p), tgt.ctypes.data_as(_i32p), int(place), int(descend), out.ctypes.data_as(_u8p),
                          weight.ctypes.data_as(_i32p), source.ctypes.data_as(_i32p), moved.ctypes.data_as(_u8p), status.ctypes.data_as(_u8p))
    assert rc == 0
    return dict(corrections=out.reshape((n,) + shape), weight=weight, source=source, moved=moved, status=status)


_cases = {}


def case(T, code, L):
    """200 errors of the oracle at p = 0.10, their syndromes and classes, the twin lift of every syndrome as the candidate; every row once per
    target class (row s * ncls + t: error s towards class t).  Computed once per shape."""
    if (code, L) not in _cases:
        _, raw, eq = orc.generate_syndromes(ORC_CODE[code], L, N_ERR, 0.1 / 3, 0.1 / 3, 0.1 / 3, hide_class=False, seed=7)
        assert np.array_equal(eq, classes(code, raw))
        defects = syndromes(code, raw)
        lifted, status, _ = lift_cpu.twin(T, code, L, defects, 1)
        assert not status.any()
        n = ncls_of(code)
        c = dict(errors=np.repeat(raw, n, axis=0), err_class=np.repeat(eq, n), defects=np.repeat(defects, n, axis=0), cand=np.repeat(lifted, n, axis=0),
                 cand_class=np.repeat(classes(code, lifted), n), cand_weight=np.repeat(weights(lifted), n), target=np.tile(np.arange(n, dtype=np.int32), N_ERR),
                 need=class_moves(T, code, L), gens=generators(code, L))
        for v in c.values():
            v.setflags(write=False)
        _cases[code, L] = c
    return _cases[code, L]


@pytest.mark.parametrize("code,L", SHAPES)
def test_class_move_table(T, code, L):
    need = class_moves(T, code, L)
    kinds = 4 if code == TORIC else 2
    assert need.max() < (1 << kinds) and not np.diag(need).any()
    chains = lift_cpu.random_errors(code, L, 48, np.random.default_rng([11, code, L]))
    seen = set()
    for m in chains:
        a = oracle_class(code, m)
        seen.add(a)
        for b in range(ncls_of(code)):
            moved = m
            for kind in range(kinds):
                if need[a, b] >> kind & 1:
                    moved = apply_kind(code, moved, kind)
            assert oracle_class(code, moved) == b, (a, b, need[a, b])
            assert np.array_equal(oracle_syndrome(code, moved), oracle_syndrome(code, m))
    assert len(seen) > 1


def test_toric_even_size_is_refused_by_name(T):
    buf = np.zeros(256, dtype=np.uint32)
    assert T.qt_class_moves(TORIC, 4, buf.ctypes.data_as(_u32p), buf.size) == 0            # no table: a logical line of even length keeps the parity class
    cand, tgt, out = np.zeros((1, 32), np.uint8), np.zeros(1, np.int32), np.zeros((1, 32), np.uint8)
    assert T.qt_corrections(TORIC, 4, 1, 1, cand.ctypes.data_as(_u8p), tgt.ctypes.data_as(_i32p), 1, 1, out.ctypes.data_as(_u8p), None, None, None, None) == -4
    lib = L_.lib()
    assert lib.qecmc_corrections(TORIC, 4, 1, 1, L_.u8(cand), L_.i32(tgt), 1, 1, L_.u8(out), None, None, None, None) == -4
    msg = lib.qecmc_last_error()
    assert b"L=4" in msg and b"even length" in msg
    cr = C.c_void_p()
    assert lib.qecmc_corrector_create(TORIC, 4, C.byref(cr)) == -4 and not cr.value
    for L in (2, 4, 6):                                                                    # the planar code has a class move at every size
        assert T.qt_class_moves(PLANAR, L, buf.ctypes.data_as(_u32p), buf.size) == 16


@pytest.mark.parametrize("place,descend", SETTINGS)
@pytest.mark.parametrize("code,L", SHAPES)
def test_properties(T, code, L, place, descend):
    c = case(T, code, L)
    got = twin(T, code, L, c["cand"], c["target"], place, descend)
    cor = got["corrections"]
    assert not got["status"].any()
    assert np.array_equal(syndromes(code, cor), c["defects"])
    assert np.array_equal(classes(code, cor), c["target"])
    assert np.array_equal(got["weight"], weights(cor))
    # the pick rule with one candidate: it is the source, moved iff it is in another class
    assert not got["source"].any()
    assert np.array_equal(got["moved"], c["cand_class"] != c["target"])
    if not descend:
        keep = got["moved"] == 0
        assert np.array_equal(cor[keep], c["cand"][keep])                                   # nothing to do: the candidate itself
    if descend:                                                                             # no generator lowers the weight
        flat = cor.reshape(len(cor), -1)
        for lo in range(0, len(flat), 256):
            after = ((flat[lo:lo + 256, None, :] ^ c["gens"][None]) != 0).sum(axis=2)
            assert np.all(after >= got["weight"][lo:lo + 256, None])
    # the algebra of success: error ^ correction is a stabilizer iff the target is the error's class -- on every row, exactly
    residual = c["errors"] ^ cor
    zero_class = oracle_class(code, np.zeros(state_shape(code, L), np.uint8))
    stabilizer = ~syndromes(code, residual).any(axis=1) & (classes(code, residual) == zero_class)
    assert np.array_equal(stabilizer, c["target"] == c["err_class"])


@pytest.mark.parametrize("code,L", SHAPES)
def test_placing_never_costs_more_than_position_zero(T, code, L):
    c = case(T, code, L)
    at0 = twin(T, code, L, c["cand"], c["target"], 0, 0)
    placed = twin(T, code, L, c["cand"], c["target"], 1, 0)
    kinds = c["need"][c["cand_class"], c["target"]]
    single = np.isin(kinds, [1, 2, 4, 8])
    assert single.sum() > N_ERR // 2
    assert np.all(placed["weight"][single] <= at0["weight"][single])
    # ... and position 0 is what place = 0 means: the candidate times the oracle's logical operators at position 0
    for s in np.flatnonzero(kinds)[:40]:
        m = c["cand"][s]
        for kind in range(4):
            if kinds[s] >> kind & 1:
                m = apply_kind(code, m, kind)
        assert np.array_equal(at0["corrections"][s], m)
    # ... and place = 1 takes the best single position, ties to the lowest
    for s in np.flatnonzero(single)[:40]:
        kind = int(kinds[s]).bit_length() - 1
        tries = [apply_kind(code, c["cand"][s], kind, p) for p in range(L)]
        best = int(np.argmin([orc.count_errors(t) for t in tries]))
        assert np.array_equal(placed["corrections"][s], tries[best])


@pytest.mark.parametrize("code,L", [(TORIC, 5), (XZZX, 5), (ROTATED, 5), (PLANAR, 5), (TORIC, 3), (ROTATED, 7)])
def test_three_candidates(T, code, L):
    """the lift and two copies of it in other classes (a logical operator somewhere, a few generators on top); some rows carry the same chain twice:
    the pick rule and its ties to the lowest index, for every target class"""
    c = case(T, code, L)
    n, n_err = ncls_of(code), 60
    rng = np.random.default_rng([5, code, L])
    base = c["cand"][::n][:n_err]
    kinds = 4 if code == TORIC else 2
    cand = np.stack([base, base, base], axis=1).copy()
    for s in range(n_err):
        for k in (1, 2):
            m = apply_kind(code, cand[s, k], int(rng.integers(kinds)), int(rng.integers(L)))
            for g in rng.integers(len(c["gens"]), size=3):
                m = m ^ c["gens"][g].reshape(m.shape)
            cand[s, k] = m
        if s % 4 == 0:
            cand[s, 2] = cand[s, 1]                                                         # a tie in class and weight: index 1 wins over 2
        if s % 4 == 1:
            cand[s, 1] = cand[s, 0]                                                         # ... index 0 over 1
    flat = cand.reshape((n_err * 3,) + cand.shape[2:])
    assert np.array_equal(syndromes(code, flat).reshape(n_err, 3, -1), np.repeat(syndromes(code, base)[:, None], 3, axis=1))
    ck, wk = classes(code, flat).reshape(n_err, 3), weights(flat).reshape(n_err, 3)
    cand_t, target = np.repeat(cand, n, axis=0), np.tile(np.arange(n, dtype=np.int32), n_err)
    ck, wk = np.repeat(ck, n, axis=0), np.repeat(wk, n, axis=0)
    inside = ck == target[:, None]
    some = inside.any(axis=1)
    want_source = np.where(some, np.argmin(np.where(inside, wk, 1 << 30), axis=1), np.argmin(wk, axis=1))   # (argmin: the first of equals)
    assert some.any() and (~some).any() and (want_source > 0).any()
    for place, descend in SETTINGS:
        got = twin(T, code, L, cand_t, target, place, descend)
        assert np.array_equal(got["source"], want_source) and np.array_equal(got["moved"], ~some)
        assert np.array_equal(classes(code, got["corrections"]), target)
        assert np.array_equal(syndromes(code, got["corrections"]), np.repeat(syndromes(code, base), n, axis=0))
        assert np.array_equal(got["weight"], weights(got["corrections"]))
        if not descend:
            keep = np.flatnonzero(some)
            assert np.array_equal(got["corrections"][keep], cand_t[keep, want_source[keep]])


def test_out_of_range_targets_leave_their_neighbours_alone(T):
    for code, L in ((TORIC, 5), (ROTATED, 5)):
        c = case(T, code, L)
        cand, target = c["cand"][:12], c["target"][:12].copy()
        good = twin(T, code, L, cand, target, 1, 1)
        target[3], target[8] = -1, ncls_of(code)
        got = twin(T, code, L, cand, target, 1, 1)
        assert got["status"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0]
        for s in (3, 8):
            assert not got["corrections"][s].any() and got["weight"][s] == -1 and got["source"][s] == -1 and got["moved"][s] == 0
        keep = [s for s in range(12) if s not in (3, 8)]
        for key in got:
            assert np.array_equal(got[key][keep], good[key][keep]), key


def test_host_checks_need_no_device():
    lib = L_.lib()
    cand, tgt, out = np.zeros((1, 18), np.uint8), np.zeros(1, np.int32), np.zeros((1, 18), np.uint8)
    cr = C.c_void_p()
    for call in (lambda: lib.qecmc_corrections(0, 3, 1, 1, None, L_.i32(tgt), 1, 1, L_.u8(out), None, None, None, None),
                 lambda: lib.qecmc_corrections(0, 3, 1, 1, L_.u8(cand), None, 1, 1, L_.u8(out), None, None, None, None),
                 lambda: lib.qecmc_corrections(0, 3, 1, 1, L_.u8(cand), L_.i32(tgt), 1, 1, None, None, None, None, None),
                 lambda: lib.qecmc_corrector_create(0, 3, None),
                 lambda: lib.qecmc_corrections_dev(None, None, None, 1, 1, 1, 1, None, None, None, None, None, None)):
        assert call() == -1 and b"NULL" in lib.qecmc_last_error()
    assert lib.qecmc_corrections(0, 3, 1, 0, L_.u8(cand), L_.i32(tgt), 1, 1, L_.u8(out), None, None, None, None) == -1 and b"K=0" in lib.qecmc_last_error()
    for code in (-1, 4):
        assert lib.qecmc_corrections(code, 3, 1, 1, L_.u8(cand), L_.i32(tgt), 1, 1, L_.u8(out), None, None, None, None) == -1 and b"code" in lib.qecmc_last_error()
        assert lib.qecmc_corrector_create(code, 3, C.byref(cr)) == -1 and b"code" in lib.qecmc_last_error()
    assert lib.qecmc_corrections(1, 4, 1, 1, L_.u8(cand), L_.i32(tgt), 1, 1, L_.u8(out), None, None, None, None) == -1 and b"odd L" in lib.qecmc_last_error()
    assert lib.qecmc_corrector_create(1, 4, C.byref(cr)) == -1 and b"odd L" in lib.qecmc_last_error()
    assert lib.qecmc_corrector_create(0, 4, C.byref(cr)) == -4                             # unsupported: also before the device lookup
    assert not cr.value
    # a valid call gets as far as the device lookup: no device, no CPU fallback
    have = L_.device_count() >= 1
    for n in (1, 0):
        assert lib.qecmc_corrections(0, 3, n, 1, L_.u8(cand), L_.i32(tgt), 1, 1, L_.u8(out), None, None, None, None) == (0 if have else -2)
    rc = lib.qecmc_corrector_create(0, 3, C.byref(cr))
    assert rc == (0 if have else -2)
    if have:
        assert lib.qecmc_corrections_dev(cr, None, None, 0, 1, 1, 1, None, None, None, None, None, None) == 0      # N == 0 succeeds
        lib.qecmc_corrector_destroy(cr)
    else:
        assert b"no CPU fallback" in lib.qecmc_last_error() and not cr.value


def test_corrections_under_sanitizers():
    """a stand-alone program (its own main) built from corrections.hpp with -fsanitize=address,undefined: builds the tables of the four codes, checks
    which (code, L) have no class move, runs the body on random candidates and on out-of-range targets; run as a child process"""
    run_selftest("corrections_asan", "corrections_selftest_asan")
