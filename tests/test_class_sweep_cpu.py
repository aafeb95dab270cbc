"""The exact class law by a frontier sweep, without a GPU: the planner and the twin of csrc/class_sweep.hpp, compiled by g++ into the host-table test
library (qt_class_sweep_info, qt_class_sweep_ops, qt_class_sweep), and the Python layer (qecmc.exact) around them.

What is pinned: the invariants of the op stream against the oracle's stencils (every generator lives in one slot from before its first qubit to after
its last, every qubit is closed once naming all its generators, slots are never shared, the width is the peak); the twin against the enumerator's twin
at every L = 3 shape and one syndrome each at xzzx / rotated L = 5, under the three weight families, and against util_exact.SurfEnumeration with
w_X != w_Y; all-ones weights give exactly 2^rank up to L = 9; a NumPy variable elimination written here, over the oracle's stencils in REVERSED
qubit order, at xzzx L = 7, rotated L = 9 and planar L = 5; Z as a function of the syndrome alone; the refusals by name.

Tolerance 1e-12 relative per class weight: all terms are positive, either side errs by about (nq + G) 2^-53 < 2e-14 at L = 9, and 1e-12 is what the
enumerator's tests use."""
import ctypes as C

import numpy as np
import pytest

import test_enumerate_cpu as E
from hostlib import run_selftest
from oracle import oracle as orc
from qecmc import _lib as L_
from qecmc import exact as ex
from test_corrections_cpu import class_moves, classes, generators
from test_corrections_cpu import load_twin as load_corrections_twin
from test_exact_cpu import ORC_API, _rand_surf
from test_syndrome_lift_cpu import ORC_CODE, PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_exact import SurfEnumeration

REQUIRED = [(XZZX, 3), (XZZX, 5), (XZZX, 7), (XZZX, 9), (ROTATED, 3), (ROTATED, 5), (ROTATED, 7), (ROTATED, 9), (PLANAR, 3), (PLANAR, 4), (PLANAR, 5),
            (PLANAR, 6), (TORIC, 3)]
NAME = {TORIC: "toric", XZZX: "xzzx", ROTATED: "rotated", PLANAR: "planar"}
INTRO, CLOSE, FORGET = 0, 1, 2
_u8p, _u32p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double)
# the three weight families in ratio form, and one weight no histogram over (n_xy, n_z) can express
FAMILIES = [ex.depolarizing_w4(0.1), ex.depolarizing_w4(0.2), ex.biased_w4(0.25, 3.0), ex.biased_w4(0.15, 100.0), ex.alpha_w4(0.3, 2.5)]
HIST_WEIGHTS = [ex.depolarizing_weight(0.1), ex.depolarizing_weight(0.2), ex.biased_weight(0.25, 3.0), ex.biased_weight(0.15, 100.0), ex.alpha_weight(0.3, 2.5)]
SKEW = np.array([1.0, 0.05, 0.011, 0.23])


def load_twin():
    """the host-table test library with the sweep's entry points (tests/test_gpu_class_sweep.py compares the GPU with it)"""
    lib = E.load_twin()
    load_corrections_twin()                                                     # (the same handle: qt_class_moves gets its signature)
    lib.qt_class_moves.restype = C.c_int
    lib.qt_class_moves.argtypes = [C.c_int, C.c_int, _u32p, C.c_int]
    lib.qt_class_sweep_info.restype = C.c_int
    lib.qt_class_sweep_info.argtypes = [C.c_int, C.c_int, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_sweep_ops.restype = C.c_int
    lib.qt_class_sweep_ops.argtypes = [C.c_int, C.c_int, _u32p, C.c_int]
    lib.qt_class_sweep.restype = C.c_int
    lib.qt_class_sweep.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _f64p, _f64p, _i32p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def info(T, code, L):
    """(rc, dict(width, ncls, nq, n_ops, rank, n_gen, lds_bytes, max_width), message)"""
    v, msg = np.zeros(8, np.int32), C.create_string_buffer(512)
    rc = T.qt_class_sweep_info(code, L, v.ctypes.data_as(_i32p), msg, 512)
    return rc, dict(zip(("width", "ncls", "nq", "n_ops", "rank", "n_gen", "lds_bytes", "max_width"), v.tolist())), msg.value


def twin(T, code, L, chains, w):
    """the host twin on chains [N, ...] -> (Z float64[N, ncls], cls int32[N])"""
    nq = int(np.prod(state_shape(code, L)))
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    w = np.ascontiguousarray(w, dtype=np.float64)
    z, cls = np.full((len(flat), 16 if code == TORIC else 4), -1.0), np.full(len(flat), 9, np.int32)
    rc = T.qt_class_sweep(code, L, len(flat), flat.ctypes.data_as(_u8p), w.ctypes.data_as(_f64p), z.ctypes.data_as(_f64p), cls.ctypes.data_as(_i32p))
    assert rc == 0, rc
    return z, cls


def ops_of(T, code, L):
    """the op stream as a list of (kind, slot, top, mask, [(slot, Pauli)], qubit)"""
    _, inf, _ = info(T, code, L)
    buf = np.zeros(4 * inf["n_ops"], np.uint32)
    assert T.qt_class_sweep_ops(code, L, buf.ctypes.data_as(_u32p), buf.size) == buf.size
    out = []
    for w0, mask, pairs, qubit in buf.reshape(-1, 4).tolist():
        pr = [((pairs >> 8 * j) & 15, (pairs >> (8 * j + 4)) & 15) for j in range((w0 >> 8) & 15)]
        out.append((w0 & 15, (w0 >> 4) & 15, (w0 >> 12) & 31, mask, [(s, xz ^ (xz >> 1)) for s, xz in pr], qubit))
    return out


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.asarray(b)


# ------------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("code,L", REQUIRED)
def test_plan_invariants(T, code, L):
    rc, inf, msg = info(T, code, L)
    assert rc == 0, msg
    gens = generators(code, L)
    print("%s L=%d: width %d, %d ops" % (NAME[code], L, inf["width"], inf["n_ops"]))
    assert inf["width"] <= 13 and inf["width"] <= inf["max_width"] and inf["lds_bytes"] == 8 << inf["width"] <= 64 * 1024
    assert inf["n_gen"] == len(gens) and inf["rank"] == (len(gens) - 2 if code == TORIC else len(gens))
    live, lifetimes, closed, peak = {}, [], [], 0                               # live: slot -> the (qubit, Pauli) pairs that named it so far
    for kind, slot, top, mask, pairs, qubit in ops_of(T, code, L):
        before = sum(1 << s for s in live)
        if kind == INTRO:
            assert slot not in live and mask == before and top > slot and mask >> top == 0
            live[slot] = set()
            peak = max(peak, len(live))
        elif kind == CLOSE:
            assert mask == before and mask >> top == 0 and len({s for s, _ in pairs}) == len(pairs)
            for s, pauli in pairs:
                assert s in live and pauli in (1, 2, 3)
                live[s].add((qubit, pauli))
            closed.append(qubit)
            assert sorted(p for _, p in pairs) == sorted(int(g[qubit]) for g in gens if g[qubit])      # all the generators that touch it
        else:
            assert kind == FORGET and slot in live and top > slot
            lifetimes.append(frozenset(live.pop(slot)))
            assert mask == sum(1 << s for s in live) and mask >> top == 0
    assert not live                                                             # the stream ends with no live slot
    assert peak == inf["width"]
    touched = [q for q in range(gens.shape[1]) if gens[:, q].any()]
    assert sorted(closed) == touched                                            # every qubit once; a cell that holds no qubit is not in the stream
    supports = [frozenset((q, int(g[q])) for q in np.flatnonzero(g)) for g in gens]
    assert sorted(map(sorted, lifetimes)) == sorted(map(sorted, supports))      # one lifetime per generator, from before its first qubit to after its last
    assert len(set(supports)) == len(supports)


def test_widths_the_planner_reports(T):
    got = {(NAME[c], L): info(T, c, L)[1]["width"] for c, L in REQUIRED}
    print(got)
    assert max(got.values()) <= 13


# ------------------------------------------------------------------------------------------------------ the twin against the enumerator's twin
_enum_twin = {}


def enum_case(T, code, L):
    """chains of one shape with their histograms from the enumerator's twin, computed once"""
    if (code, L) not in _enum_twin:
        chains = E.whole(T, code, L)[0] if L == 3 else _rand_surf(50 + ORC_CODE[code], 5, 0.2)[None]
        hist = E.whole(T, code, L)[1] if L == 3 else E.twin(T, code, L, chains)[0]
        _enum_twin[code, L] = (chains, hist)
    return _enum_twin[code, L]


@pytest.mark.parametrize("code,L", [(TORIC, 3), (PLANAR, 3), (XZZX, 3), (ROTATED, 3), (XZZX, 5), (ROTATED, 5)])
def test_twin_is_the_enumerators_twin(T, code, L):
    chains, hist = enum_case(T, code, L)
    for w4, wh in zip(FAMILIES, HIST_WEIGHTS):
        z, cls = twin(T, code, L, chains, w4)
        want = ex.class_weights(hist, wh)
        print(NAME[code], L, "max relative difference %.3g" % rel(z, want).max())
        assert rel(z, want).max() < 1e-12
        assert np.array_equal(cls, classes(code, chains))


@pytest.mark.parametrize("code", [XZZX, ROTATED])
def test_twin_with_unequal_x_and_y_weights_is_the_brute_force(T, code):
    init = _rand_surf(6)
    cfg = SurfEnumeration(ORC_CODE[code], init, ORC_API).cfg                    # [4, 2^8, 9]
    want = SKEW[cfg].prod(axis=-1).sum(axis=1)
    z, _ = twin(T, code, 3, init[None], SKEW)
    assert rel(z[0], want).max() < 1e-12
    swapped, _ = twin(T, code, 3, init[None], SKEW[[0, 2, 1, 3]])
    assert rel(swapped[0], want).max() > 1e-3                                   # (the case tells X from Y)


@pytest.mark.parametrize("code,L", REQUIRED)
def test_all_ones_weights_count_the_group(T, code, L):
    """w = (1, 1, 1, 1): every class weight is the number of group elements, 2^rank -- 2^80 at L = 9, 2^16 on the torus after the division by 4 --,
    exactly: sums of equal powers of two"""
    _, inf, _ = info(T, code, L)
    chains = random_errors(code, L, 2, np.random.default_rng([5, code, L]))
    z, _ = twin(T, code, L, chains, np.ones(4))
    assert inf["rank"] == {TORIC: 2 * L * L - 2, PLANAR: 2 * L * (L - 1)}.get(code, L * L - 1)
    assert np.all(z == 2.0 ** inf["rank"])


# ------------------------------------------------------------------------------------------------------ an independent elimination
def eliminate(gens, chain, w4, order=None):
    """sum over the subsets of the generators (byte chains [G, nq], the oracle's stencils) of prod_q w4[chain_q ^ the generators of the subset at q]
    by variable elimination over the qubits in `order` (default: REVERSED): a NumPy array with one axis per open generator"""
    n_gen, nq = gens.shape
    left = (gens != 0).sum(axis=1)
    axes, A = [], np.ones(())
    for q in (range(nq - 1, -1, -1) if order is None else order):
        here = [g for g in range(n_gen) if gens[g, q]]
        if not here:
            continue
        for g in here:
            if g not in axes:
                axes.append(g)
                A = np.stack([A, A], axis=-1)
        pauli = np.full((2,) * len(here), int(chain[q]))
        for i, g in enumerate(here):
            sel = np.arange(2).reshape([2 if j == i else 1 for j in range(len(here))])
            pauli = pauli ^ (sel * int(gens[g, q]))                             # (byte values XOR as the Pauli product)
        factor = w4[pauli]
        where = [axes.index(g) for g in here]
        shape = [1] * len(axes)
        for i, a in enumerate(where):
            shape[a] = 2
        A = A * factor.transpose(np.argsort(where)).reshape(shape)
        for g in here:
            left[g] -= 1
            if left[g] == 0:
                a = axes.index(g)
                A = A.sum(axis=a)
                axes.pop(a)
        assert len(axes) <= 16, "the order of this test opens too many generators at once"
    assert not axes
    return float(A)


def column_major(code, L):
    """the planar code's qubits column by column of the lattice in half steps (layer 1 lies half a step down and right of layer 0), last column first"""
    assert code == PLANAR
    key = lambda q: (2 * (q % L) + q // (L * L), 2 * (q % (L * L) // L) + q // (L * L))
    return sorted(range(2 * L * L), key=key, reverse=True)


@pytest.mark.parametrize("code,L", [(XZZX, 7), (ROTATED, 9), (PLANAR, 5)])
def test_twin_is_an_independent_elimination(T, code, L):
    chains = random_errors(code, L, 3, np.random.default_rng([8, code, L]))
    gens = generators(code, L)
    w4 = ex.depolarizing_w4(0.1) if code != ROTATED else ex.biased_w4(0.1, 3.0)
    z, cls = twin(T, code, L, chains, w4)
    assert np.array_equal(cls, classes(code, chains))
    for s, m in enumerate(chains):
        reps = E.class_chains(code, m)                                          # one chain per class, by the oracle's logical operators and class function
        want = np.array([eliminate(gens, r, w4, column_major(code, L) if code == PLANAR else None) for r in reps])
        print(NAME[code], L, "syndrome", s, "max relative difference %.3g" % rel(z[s], want).max())
        assert rel(z[s], want).max() < 1e-12


def test_the_elimination_of_this_file_is_a_brute_force_at_L3():
    init = _rand_surf(7)
    cfg = SurfEnumeration(ORC_CODE[XZZX], init, ORC_API).cfg
    want = SKEW[cfg].prod(axis=-1).sum(axis=1)
    got = [eliminate(generators(XZZX, 3), cfg[c, 0], SKEW) for c in range(4)]
    assert rel(got, want).max() < 1e-13


# ------------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("code,L", [(TORIC, 3), (PLANAR, 4), (XZZX, 5), (ROTATED, 7)])
def test_Z_is_a_function_of_the_syndrome(T, code, L):
    chains = random_errors(code, L, 3, np.random.default_rng([6, code, L]))
    z, cls = twin(T, code, L, chains, SKEW)
    assert np.array_equal(cls, classes(code, chains))                           # class_out is qecmc_eq_class (the oracle's class function)
    gens, rng = generators(code, L), np.random.default_rng([7, code, L])
    moved = chains.copy()
    for s in range(len(moved)):
        for g in rng.integers(len(gens), size=7):
            moved[s] ^= gens[g].reshape(moved[s].shape)
    z2, c2 = twin(T, code, L, moved, SKEW)
    assert rel(z2, z).max() < 1e-12 and np.array_equal(c2, cls)
    # a logical operator away: the columns are indexed by the class itself, so the same Z and only the class of the input moves -- to the class the
    # class-move table names
    ncls = z.shape[1]
    other = np.stack([E.class_chains(code, m)[(c + 1) % ncls].reshape(m.shape) for m, c in zip(chains, cls)])
    z3, c3 = twin(T, code, L, other, SKEW)
    assert rel(z3, z).max() < 1e-12 and np.array_equal(c3, (cls + 1) % ncls)
    need = class_moves(T, code, L)
    assert need.shape == (ncls, ncls) and all(need[a, a] == 0 for a in range(ncls))


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(T):
    for code, L in [(XZZX, 4), (ROTATED, 6), (TORIC, 1), (TORIC, 65), (-1, 3), (4, 3)]:
        assert info(T, code, L)[0] == -1, (code, L)
    for code, L, frag in [(TORIC, 4, b"even length"), (TORIC, 5, b"21 generators wide"), (XZZX, 11, b"14 generators wide"), (ROTATED, 11, b"14 generators wide"),
                          (PLANAR, 7, b"14 generators wide"), (TORIC, 63, b"generators wide"), (PLANAR, 64, b"generators wide")]:
        rc, _, msg = info(T, code, L)
        assert rc == -4 and frag in msg, (code, L, msg)
    chains, z = np.zeros((1, 9), np.uint8), np.zeros((1, 4))
    call = lambda w, c=chains, out=z: T.qt_class_sweep(XZZX, 3, 1, None if c is None else c.ctypes.data_as(_u8p), None if w is None else np.array(w, np.float64).ctypes.data_as(_f64p),
                                                        None if out is None else out.ctypes.data_as(_f64p), None)
    assert call([1, 1, 1, 1]) == 0
    for bad in ([1, 0, 1, 1], [1, 1, -0.5, 1], [1, 1, 1, np.nan], [np.inf, 1, 1, 1], [0, 1, 1, 1]):
        assert call(bad) == -1, bad
    assert call(None) == -1 and call([1, 1, 1, 1], c=None) == -1 and call([1, 1, 1, 1], out=None) == -1


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    chains, z, cls = np.zeros((1, 9), np.uint8), np.zeros((1, 4)), np.zeros(1, np.int32)
    zp = z.ctypes.data_as(_f64p)
    wp = lambda w: np.array(w, np.float64).ctypes.data_as(_f64p)
    ones = wp([1, 1, 1, 1])
    assert lib.qecmc_class_sweep(XZZX, 3, 1, None, ones, zp, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep(XZZX, 3, 1, L_.u8(chains), None, zp, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep(XZZX, 3, 1, L_.u8(chains), ones, None, None) == -1 and b"NULL" in lib.qecmc_last_error()
    for bad in ([1, 0, 1, 1], [1, 1, -1, 1], [1, 1, 1, np.nan], [1, np.inf, 1, 1]):
        assert lib.qecmc_class_sweep(XZZX, 3, 1, L_.u8(chains), wp(bad), zp, None) == -1 and b"finite and > 0" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep(XZZX, 4, 1, L_.u8(chains), ones, zp, None) == -1 and b"odd L" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep(7, 3, 1, L_.u8(chains), ones, zp, None) == -1 and b"code" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep(TORIC, 4, 1, L_.u8(chains), ones, zp, None) == -4 and b"even length" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep(TORIC, 5, 1, L_.u8(chains), ones, zp, None) == -4 and b"generators wide" in lib.qecmc_last_error()
    v = [C.c_int32() for _ in range(4)]
    assert lib.qecmc_class_sweep_info(ROTATED, 9, *[C.byref(x) for x in v]) == 0 and [x.value for x in v][1:3] == [4, 81] and v[0].value <= 13
    assert lib.qecmc_class_sweep_info(TORIC, 3, None, None, None, None) == 0
    assert lib.qecmc_class_sweep_info(TORIC, 5, None, None, None, None) == -4
    assert ex.sweep_info("planar", 6)["nq"] == 72
    # a valid call gets as far as the device lookup: no device, no CPU fallback
    have = L_.device_count() >= 1
    for n in (1, 0):
        assert lib.qecmc_class_sweep(XZZX, 3, n, L_.u8(chains), ones, zp, L_.i32(cls)) == (0 if have else -2)
    if not have:
        assert b"no CPU fallback" in lib.qecmc_last_error()
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.class_sweep("xzzx", chains.reshape(1, 3, 3), np.ones(4))
    with pytest.raises(ValueError, match="device 0"):
        ex.class_sweep("xzzx", chains.reshape(1, 3, 3), np.ones(4), device=1)
    with pytest.raises(ValueError, match="four weights"):
        ex.class_sweep("xzzx", chains.reshape(1, 3, 3), np.ones(3))


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_auto_is_the_enumerator_wherever_it_takes_the_shape(T):
    for code, L in E.SUPPORTED:
        assert ex.resolve_method(NAME[code], L) == "enumerate" and ex.resolve_method(code, L, "sweep") == "sweep"
    for code, L in [(XZZX, 7), (XZZX, 9), (ROTATED, 7), (ROTATED, 9), (PLANAR, 5), (PLANAR, 6)]:
        assert ex.resolve_method(NAME[code], L) == "sweep"
    assert ex.resolve_method("xzzx", 4) == "enumerate"                          # (not a shape: the enumerator's refusal is the one to report)
    with pytest.raises(ValueError):
        ex.resolve_method("xzzx", 3, "best")
    # with a histogram the method is the enumerator's, whatever is asked: the numbers of before
    chains, hist = enum_case(T, ROTATED, 3)
    for kw in (dict(p=0.2), dict(p=0.25, eta=3.0), dict(p=0.3, alpha=2.5)):
        a = ex.exact_class_probabilities("rotated", None, hist=hist, **kw)
        assert np.array_equal(a, ex.exact_class_probabilities("rotated", None, hist=hist, method="enumerate", **kw))
        assert np.array_equal(a, ex.exact_class_probabilities("rotated", None, hist=hist, method="auto", **kw))
    with pytest.raises(ValueError):
        ex.exact_class_probabilities("rotated", None, 0.1, eta=2.0, alpha=2.0, hist=hist)
    with pytest.raises(ValueError):
        ex.exact_class_probabilities("rotated", None, 0.1, hist=hist, method="best")


@pytest.mark.parametrize("code,L", [(TORIC, 3), (PLANAR, 3), (XZZX, 3), (ROTATED, 3), (XZZX, 5), (ROTATED, 5)])
def test_the_sweeps_law_is_the_enumerators(T, code, L):
    """the w4 helpers against the count weights, through the two twins: what method "sweep" normalises against what method "enumerate" does"""
    chains, hist = enum_case(T, code, L)
    for w4, kw in ((ex.depolarizing_w4(0.2), dict(p=0.2)), (ex.biased_w4(0.25, 3.0), dict(p=0.25, eta=3.0)), (ex.alpha_w4(0.3, 2.5), dict(p=0.3, alpha=2.5))):
        if code == TORIC and len(kw) > 1:
            continue
        z, _ = twin(T, code, L, chains, w4)
        want = ex.exact_class_probabilities(NAME[code], None, hist=hist, **kw)
        assert np.abs(z / z.sum(axis=1, keepdims=True) - want).max() < 1e-12
    assert ex.depolarizing_w4(0.2)[0] == ex.biased_w4(0.2, 3.0)[0] == ex.alpha_w4(0.2, 3.0)[0] == 1.0


def test_a_row_whose_weights_all_underflow_raises():
    hist = np.zeros((1, 4, 10, 10), np.uint64)
    hist[0, :, 9, 0] = 1
    with pytest.raises(FloatingPointError):
        ex.exact_class_probabilities("xzzx", None, 1e-80, hist=hist)


# ------------------------------------------------------------------------------------------------------ the sanitizers
def test_sweep_under_sanitizers():
    """a stand-alone program (its own main) built from class_sweep.hpp with -fsanitize=address,undefined: the plan of every (code, L), accepted or
    refused, and the twin on random chains of every plan up to width 10; run as a child process"""
    run_selftest("sweep_asan", "class_sweep_selftest_asan")
