"""The three sweeps under a weight per (syndrome, qubit), without a GPU: the twins of csrc/class_sweep_site.hpp, compiled by g++ into the host-table
test library (qt_class_sweep_site, qt_class_sweep_cut_site, qt_class_sweep_tiled_site), and the Python layer (qecmc.exact, qecmc.harness) around them.

What is pinned: util_site.eliminate_site -- the NumPy elimination of tests/test_class_sweep_cpu.py with the factor of a qubit read from its own row --
against a brute force over the whole group; the three twins against it on every route; constant rows against the uniform twins BIT FOR BIT; the row
a syndrome reads; Z as a function of the syndrome alone; the pure-erasure channel, where every class weight is 0 or one power of two, exactly; cells
that hold no qubit; every refusal by name; the shapes and the routing of the Python layer; the twins under the sanitizers.

Tolerances: 1e-13 relative for the elimination against the brute force and 1e-12 relative per class weight for a twin against the elimination, as
tests/test_class_sweep_cpu.py -- all terms are non-negative and either side errs by about (nq + G) 2^-53."""
import ctypes as C

import numpy as np
import pytest

import test_class_sweep_cpu as S
import test_class_sweep_cut_cpu as SC
import test_class_sweep_tiled_cpu as ST
import test_enumerate_cpu as E
import test_syndrome_lift_cpu as lift_cpu
from hostlib import run_selftest
from qecmc import _lib as L_
from qecmc import exact as ex
from qecmc import harness
from test_corrections_cpu import classes, generators
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_sectors import order_for
from util_site import eliminate_site, random_site_weights

NAME = S.NAME
_u8p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
# the small tiled plan: from test_class_sweep_tiled_cpu.ACCEPTED, a state vector of 2^8 entries in tiles of 2^4 -- CLOSE pairs on slots fixed in the tile
SMALL_TILED = (XZZX, 5, 0, 4)
assert SMALL_TILED in ST.ACCEPTED
# the smallest tiled plan in which one launch group takes two workspace passes: five held generators, 2^16 units in a group of 128 syndromes
HELD_TILED = (TORIC, 3, 8, 4)
# (route, code, L, widths): widths are (), (lds_width,) or (hbm_width, tile_width)
ROUTES = [("sweep", XZZX, 7, ()), ("sweep", PLANAR, 5, ()), ("cut", ROTATED, 11, (0,)), ("cut", TORIC, 3, (4,)), ("tiled", ROTATED, 13, (0, 0)),
          ("tiled",) + SMALL_TILED[:2] + (SMALL_TILED[2:],), ("tiled",) + HELD_TILED[:2] + (HELD_TILED[2:],)]
SMALL = [("sweep", XZZX, 5, ()), ("sweep", PLANAR, 4, ()), ("cut", TORIC, 3, (4,)), ("cut", PLANAR, 3, (3,)), ("tiled",) + SMALL_TILED[:2] + (SMALL_TILED[2:],),
         ("tiled",) + HELD_TILED[:2] + (HELD_TILED[2:],)]
ENTRY = {"sweep": "qt_class_sweep_site", "cut": "qt_class_sweep_cut_site", "tiled": "qt_class_sweep_tiled_site"}
UNIFORM = {"sweep": S.twin, "cut": SC.twin, "tiled": ST.twin}
W4 = np.array([1.0, 0.043, 0.019, 0.21])


def load_twin():
    """the host-table test library with the site twins (tests/test_gpu_class_sweep_site.py compares the GPU with it)"""
    lib = ST.load_twin()
    head = [C.c_int, C.c_int, C.c_uint64, _u8p, _f64p, C.c_uint64]
    tail = [_f64p, _i32p, C.c_char_p, C.c_int]
    for route, widths in (("sweep", 0), ("cut", 1), ("tiled", 2)):
        fn = getattr(lib, ENTRY[route])
        fn.restype, fn.argtypes = C.c_int, head + [C.c_int] * widths + tail
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def nq_of(code, L):
    return int(np.prod(state_shape(code, L)))


def call(T, route, code, L, chains, wq, widths=(), rows=None, n=None, z=True):
    """one site twin on chains [N, ...] and wq [rows, ...] -> (rc, message, Z float64[N, ncls], cls int32[N]); None for a NULL buffer"""
    nq = nq_of(code, L)
    flat = None if chains is None else np.ascontiguousarray(chains, dtype=np.uint8)
    flat = flat if flat is None or flat.size % nq else flat.reshape(-1, nq)     # (rows of another length are taken as they are: a refused (code, L) reads none)
    n = len(flat) if n is None else n
    w = None if wq is None else np.ascontiguousarray(wq, dtype=np.float64)
    w = w if w is None or w.size % (4 * nq) else w.reshape(-1, nq, 4)
    rows = len(w) if rows is None else rows
    out, cls, msg = np.full((n, 16 if code == TORIC else 4), -1.0), np.full(n, 9, np.int32), C.create_string_buffer(512)
    rc = getattr(T, ENTRY[route])(code, L, n, None if flat is None else flat.ctypes.data_as(_u8p), None if w is None else w.ctypes.data_as(_f64p), rows,
                                  *[int(x) for x in widths], out.ctypes.data_as(_f64p) if z else None, cls.ctypes.data_as(_i32p), msg, 512)
    return rc, msg.value, out, cls


def twin(T, route, code, L, chains, wq, widths=()):
    """the site twin of one route -> (Z, cls); wq [..., 4] one table, or [N, ..., 4]"""
    rc, msg, z, cls = call(T, route, code, L, chains, wq, widths)
    assert rc == 0, (rc, msg)
    return z, cls


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([61, code, L, seed]))


def tables_of(code, L, n, seed=0):
    """n tables of random weights, log-uniform in [1e-3, 1]: float64[n, nq, 4]"""
    return random_site_weights(np.random.default_rng([67, code, L, seed]), (n, nq_of(code, L)))


def scale_of(code, L):
    """every group element is met 2^(G - rank) times by a sum over the subsets of the generator table: 4 on the torus, 1 elsewhere"""
    return 0.25 if code == TORIC else 1.0


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------------------------ 1. the elimination of util_site.py
@pytest.mark.parametrize("code", [XZZX, TORIC])
def test_eliminate_site_is_a_brute_force_at_L3(code):
    gens = generators(code, 3)
    chain = chains_of(code, 3, 3)[2].reshape(-1)
    wq = tables_of(code, 3, 1)[0]
    group = E.span(gens) ^ chain                                                # every subset of the generator table on the chain: [2^G, nq]
    want = wq[np.arange(gens.shape[1]), group].prod(axis=1).sum()
    got = eliminate_site(gens, chain, wq, order_for(code, 3))
    assert abs(got - want) / want < 1e-13
    assert abs(eliminate_site(gens, chain, wq[::-1].copy(), order_for(code, 3)) - want) / want > 1e-3       # (the case tells the rows apart)


# ------------------------------------------------------------------------------------------------------ 2. the twins against it
@pytest.mark.parametrize("route,code,L,widths", ROUTES)
def test_site_twin_is_an_independent_elimination(T, route, code, L, widths):
    chains, wq = chains_of(code, L, 2), tables_of(code, L, 2)
    if code == PLANAR:
        wq.reshape((2,) + state_shape(code, L) + (4,))[:, 1, -1, :] = np.nan    # (cells that hold no qubit: not read)
        wq.reshape((2,) + state_shape(code, L) + (4,))[:, 1, :, -1] = np.nan
    z, cls = twin(T, route, code, L, chains, wq, widths)
    assert np.array_equal(cls, classes(code, chains))
    gens = generators(code, L)
    for s, m in enumerate(chains):
        reps = E.class_chains(code, m)
        want = np.array([eliminate_site(gens, r, np.nan_to_num(wq[s]), order_for(code, L)) for r in reps]) * scale_of(code, L)
        print(route, NAME[code], L, "syndrome", s, "max relative difference %.3g" % S.rel(z[s], want).max())
        assert S.rel(z[s], want).max() < 1e-12
    if (route, code, L) + tuple(widths) == ("tiled",) + SMALL_TILED:            # the small tiled plan does have CLOSE pairs on slots fixed in the tile
        ops, segs = ST.ops_of(T, *SMALL_TILED), ST.segments_of(T, *SMALL_TILED)
        assert any(not (sg["tile"] >> slot) & 1 for sg in segs for o in range(sg["op_first"], sg["op_first"] + sg["op_count"]) if ops[o][0] == S.CLOSE
                   for slot, _ in ops[o][4])


# ------------------------------------------------------------------------------------------------------ 3. constant rows
@pytest.mark.parametrize("route,code,L,widths", SMALL)
def test_constant_rows_are_the_uniform_twin_bit_for_bit(T, route, code, L, widths):
    chains = chains_of(code, L, 3)
    want, cls = UNIFORM[route](T, code, L, chains, W4, *widths)
    for rows in (1, 3):
        z, c = twin(T, route, code, L, chains, np.broadcast_to(W4, (rows, nq_of(code, L), 4)), widths)
        assert same_bits(z, want) and np.array_equal(c, cls), rows


# ------------------------------------------------------------------------------------------------------ 4. the row a syndrome reads
@pytest.mark.parametrize("route,code,L,widths", SMALL)
def test_row_s_belongs_to_syndrome_s(T, route, code, L, widths):
    chains, wq = chains_of(code, L, 3), tables_of(code, L, 3)
    z, _ = twin(T, route, code, L, chains, wq, widths)
    for s in range(3):
        alone, _ = twin(T, route, code, L, chains, wq[s], widths)
        assert same_bits(alone[s], z[s])
    permuted, _ = twin(T, route, code, L, chains, wq[[1, 2, 0]], widths)
    assert all(not same_bits(permuted[s], z[s]) for s in range(3))


# ------------------------------------------------------------------------------------------------------ 5. structure
@pytest.mark.parametrize("route,code,L,widths", SMALL)
def test_Z_is_a_function_of_the_syndrome_under_site_weights(T, route, code, L, widths):
    chains, wq = chains_of(code, L, 3, seed=1), tables_of(code, L, 3, seed=1)
    z, cls = twin(T, route, code, L, chains, wq, widths)
    gens, rng = generators(code, L), np.random.default_rng([71, code, L])
    moved = chains.copy()
    for s in range(len(moved)):
        for g in rng.integers(len(gens), size=7):
            moved[s] ^= gens[g].reshape(moved[s].shape)
    z2, c2 = twin(T, route, code, L, moved, wq, widths)
    assert S.rel(z2, z).max() < 1e-12 and np.array_equal(c2, cls)
    # a logical operator away: the columns are indexed by the class itself, so the same Z and only the class of the input moves
    ncls = z.shape[1]
    other = np.stack([E.class_chains(code, m)[(c + 1) % ncls].reshape(m.shape) for m, c in zip(chains, cls)])
    z3, c3 = twin(T, route, code, L, other, wq, widths)
    assert S.rel(z3, z).max() < 1e-12 and np.array_equal(c3, (cls + 1) % ncls)


# ------------------------------------------------------------------------------------------------------ 6. pure erasure
# (code, L) -> the seed of its 20 shots, chosen here on the CPU: at least 5 shots with one non-zero class and at least 1 with several (of seeds 0 .. 59
# the first that gives two shots with several classes: 18 + 2 for both shapes)
ERASURE_SEEDS = {(ROTATED, 5): 0, (PLANAR, 4): 1}
_erasure = {}


def erasure_case(T, code, L, n=20):
    """n shots of the pure-erasure channel at p_erase = 0.25, computed once: dict(erased bool[n, ...], errors: uniform Paulis on the erased cells,
    chains: the start chains the syndrome lift's twin gives the bare syndromes, wq: (1, 0, 0, 0) off the set and (1, 1, 1, 1) on it, eq_true)"""
    if (code, L) not in _erasure:
        rng = np.random.default_rng([73, code, L, ERASURE_SEEDS[code, L]])
        erased = harness.draw_erasures(code, L, n, 0.25, rng)
        errors = harness.apply_erasures(np.zeros((n,) + state_shape(code, L), np.uint8), erased, rng)
        assert not errors[~erased].any() and set(np.unique(errors[erased]).tolist()) == {0, 1, 2, 3}
        if code == PLANAR:
            assert not erased[:, 1, -1, :].any() and not erased[:, 1, :, -1].any()
        defects = np.stack([lift_cpu.oracle_syndrome(code, m) for m in errors])
        chains, status, _ = lift_cpu.twin(T, code, L, defects, 1)
        assert not status.any()
        wq = ex.erasure_site_w4(np.array([1.0, 0.0, 0.0, 0.0]), erased)
        _erasure[code, L] = dict(erased=erased, errors=errors, chains=chains, wq=wq, eq_true=classes(code, errors))
    return _erasure[code, L]


def check_erasure_law(z, eq_true):
    """the exact assertions of the pure-erasure channel on Z float64[n, ncls] -> (shots with one non-zero class, shots with several)"""
    one = several = 0
    for s, row in enumerate(z):
        live = row[row != 0.0]
        assert len(live) >= 1 and np.all(live == live[0]) and np.frexp(live[0])[0] == 0.5, (s, row)     # 0, or one common power of two
        assert row[eq_true[s]] != 0.0, (s, row)
        if len(live) == 1:
            assert int(np.argmax(row)) == int(eq_true[s])
            one += 1
        else:
            several += 1
    return one, several


@pytest.mark.parametrize("code,L", sorted(ERASURE_SEEDS))
def test_pure_erasure_is_exact(T, code, L):
    case = erasure_case(T, code, L)
    z, _ = twin(T, "sweep", code, L, case["chains"], case["wq"])
    one, several = check_erasure_law(z, case["eq_true"])
    print(NAME[code], L, "shots with one non-zero class:", one, "with several:", several)
    assert one >= 5 and several >= 1


# ------------------------------------------------------------------------------------------------------ 7. cells that hold no qubit
def test_the_planar_codes_unused_cells_are_not_read():
    T = load_twin()
    for route, L, widths in (("sweep", 4, ()), ("cut", 3, (3,)), ("tiled", 4, (6, 5))):
        chains, wq = chains_of(PLANAR, L, 2), tables_of(PLANAR, L, 2).reshape(2, 2, L, L, 4)
        want, _ = twin(T, route, PLANAR, L, chains, wq, widths)
        dirty = wq.copy()
        dirty[:, 1, -1, :] = np.nan
        dirty[:, 1, :, -1] = [-1.0, np.inf, 0.0, np.nan]
        got, _ = twin(T, route, PLANAR, L, chains, dirty, widths)
        assert same_bits(got, want)
        dirty[1, 1, 0, 0, 3] = np.nan                                           # a qubit: refused by name
        rc, msg, _, _ = call(T, route, PLANAR, L, chains, dirty, widths)
        assert rc == -1 and b"wq[row 1][qubit %d][Z]=nan" % (L * L) in msg, msg


# ------------------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("route,widths", [("sweep", ()), ("cut", (0,)), ("tiled", (0, 0))])
def test_refusals_by_name(T, route, widths):
    chains, wq = np.zeros((2, 9), np.uint8), np.ones((2, 9, 4))
    ok = lambda **kw: call(T, route, kw.pop("code", XZZX), kw.pop("L", 3), kw.pop("chains", chains), kw.pop("wq", wq), kw.pop("widths", widths), **kw)
    assert ok()[0] == 0 and ok(wq=wq[:1])[0] == 0
    for kw in (dict(chains=None, n=2), dict(wq=None, rows=2), dict(z=False)):
        rc, msg, _, _ = ok(**kw)
        assert rc == -1 and b"NULL" in msg, kw
    for rows in (0, 3, 7):
        rc, msg, _, _ = ok(wq=np.ones((8, 9, 4)), rows=rows)
        assert rc == -1 and b"wq_rows=%d" % rows in msg and b"N=2" in msg
    assert ok(chains=chains[:0], wq=wq, rows=7)[0] == 0                         # N == 0 succeeds, whatever wq_rows
    for bad, shown in ((-0.5, b"-0.5"), (np.nan, b"nan"), (np.inf, b"inf"), (-np.inf, b"-inf")):
        w = wq.copy()
        w[1, 4, 2] = bad
        rc, msg, _, _ = ok(wq=w)
        assert rc == -1 and b"wq[row 1][qubit 4][Y]=" + shown in msg and b"finite and >= 0" in msg, msg
        assert ok(wq=w[:1])[0] == 0                                             # (row 0 alone is clean)
    w = wq.copy()
    w[0, 7] = 0.0
    rc, msg, _, _ = ok(wq=w)
    assert rc == -1 and b"wq[row 0][qubit 7]" in msg and b"all zero" in msg
    w[0, 7, 3] = 1e-300                                                          # zero is allowed: three of four
    assert ok(wq=w)[0] == 0
    # the sibling's refusals, with its code and message
    for code, L in [(XZZX, 4), (TORIC, 1), (-1, 3), (4, 3)]:
        assert ok(code=code, L=L)[0] == -1, (code, L)
    rc, msg, _, _ = ok(code=TORIC, L=4, chains=np.zeros((2, 32), np.uint8), wq=np.ones((2, 32, 4)))
    assert rc == -4 and b"even length" in msg
    sibling = {"sweep": lambda: S.info(T, TORIC, 5), "cut": lambda: SC.info(T, TORIC, 9, 0), "tiled": lambda: ST.info(T, TORIC, 9, 0, 0)}[route]()
    L = 5 if route == "sweep" else 9
    rc, msg, _, _ = ok(code=TORIC, L=L, chains=np.zeros((2, 2 * L * L), np.uint8), wq=np.ones((2, 2 * L * L, 4)))
    assert (rc, msg) == (sibling[0], sibling[2]) and rc == -4 and b"generators wide" in msg
    if route == "cut":
        rc, msg, _, _ = ok(widths=(15,))
        assert (rc, msg) == (SC.info(T, XZZX, 3, 15)[0], SC.info(T, XZZX, 3, 15)[2]) and rc == -1 and b"lds_width=15" in msg
    if route == "tiled":
        for hw, tw, frag in ((0, 3, b"tile_width=3"), (25, 0, b"hbm_width=25")):
            rc, msg, _, _ = ok(widths=(hw, tw))
            assert (rc, msg) == (ST.info(T, XZZX, 3, hw, tw)[0], ST.info(T, XZZX, 3, hw, tw)[2]) and rc == -1 and frag in msg


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    chains, z, cls = np.zeros((2, 9), np.uint8), np.zeros((2, 4)), np.zeros(2, np.int32)
    zp, ones = z.ctypes.data_as(_f64p), np.ones((2, 9, 4))
    wp = lambda w: np.ascontiguousarray(w, np.float64).ctypes.data_as(_f64p)
    entries = [(lib.qecmc_class_sweep_site, ()), (lib.qecmc_class_sweep_cut_site, (0,)), (lib.qecmc_class_sweep_tiled_site, (0, 0))]
    have = L_.device_count() >= 1
    for fn, widths in entries:
        run = lambda code=XZZX, L=3, n=2, c=L_.u8(chains), w=wp(ones), rows=2, out=zp, wd=widths: fn(code, L, n, c, w, rows, *wd, out, None)
        for kw in (dict(c=None), dict(w=None), dict(out=None)):
            assert run(**kw) == -1 and b"NULL" in lib.qecmc_last_error()
        assert run(rows=3) == -1 and b"wq_rows=3" in lib.qecmc_last_error()
        for bad in (-1.0, np.nan, np.inf):
            w = ones.copy()
            w[1, 8, 1] = bad
            assert run(w=wp(w)) == -1 and b"wq[row 1][qubit 8][X]" in lib.qecmc_last_error() and b"finite and >= 0" in lib.qecmc_last_error()
        w = ones.copy()
        w[0, 2] = 0.0
        assert run(w=wp(w)) == -1 and b"wq[row 0][qubit 2]" in lib.qecmc_last_error() and b"all zero" in lib.qecmc_last_error()
        assert run(L=4) == -1 and b"odd L" in lib.qecmc_last_error()
        assert run(code=7) == -1 and b"code" in lib.qecmc_last_error()
        assert run(code=TORIC, L=4) == -4 and b"even length" in lib.qecmc_last_error()
        assert run(code=TORIC, L=9) == -4 and b"generators wide" in lib.qecmc_last_error()
        # a valid call gets as far as the device lookup: no device, no CPU fallback -- also with N == 0 and with zero weights
        w = ones.copy()
        w[:, :, 1:] = 0.0
        for n, tab in ((2, ones), (0, ones), (2, w)):
            assert fn(XZZX, 3, n, L_.u8(chains), wp(tab), 2, *widths, zp, L_.i32(cls)) == (0 if have else -2)
        if not have:
            assert b"no CPU fallback" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep_cut_site(XZZX, 3, 2, L_.u8(chains), wp(ones), 2, 15, zp, None) == -1 and b"lds_width=15" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep_tiled_site(XZZX, 3, 2, L_.u8(chains), wp(ones), 2, 0, 3, zp, None) == -1 and b"tile_width=3" in lib.qecmc_last_error()
    if not have:
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.class_sweep_site("xzzx", chains.reshape(2, 3, 3), ones)


# ------------------------------------------------------------------------------------------------------ 9. the Python layer
def test_shapes_of_site_weights():
    for code, L, matrix in ((L_.XZZX, 3, (3, 3)), (L_.TORIC, 3, (2, 3, 3)), (L_.PLANAR, 4, (2, 4, 4))):
        nq = int(np.prod(matrix))
        base = np.arange(5 * nq * 4, dtype=np.float64).reshape(5, nq, 4)
        for shape, rows in ((matrix + (4,), 1), ((nq, 4), 1), ((5,) + matrix + (4,), 5), ((5, nq, 4), 5)):
            wq, got = ex._as_site_weights(code, base[:rows].reshape(shape), L, 5)
            assert got == rows and wq.shape == (rows, nq, 4) and wq.dtype == np.float64 and wq.flags.c_contiguous and np.array_equal(wq, base[:rows])
        for shape in ((4,), matrix, (nq,), matrix + (3,), (nq, 5), (4,) + matrix + (4,), (6, nq, 4), (nq + 1, 4), (5,) + matrix[::-1][:-1] + (7, 4)):
            with pytest.raises(ValueError, match="site_weights of shape"):
                ex._as_site_weights(code, np.ones(shape), L, 5)
    assert ex._as_site_weights(L_.ROTATED, np.ones((1, 3, 3, 4)), 3, 1)[1] == 1 and ex._as_site_weights(L_.ROTATED, np.ones((1, 9, 4)), 3, 5)[1] == 1
    chains = np.zeros((2, 3, 3), np.uint8)
    with pytest.raises(ValueError, match="site_weights of shape"):
        ex.class_sweep_site("xzzx", chains, np.ones((3, 9, 4)))
    with pytest.raises(ValueError, match="method="):
        ex.class_sweep_site("xzzx", chains, np.ones((9, 4)), method="enumerate")


def test_auto_is_the_first_route_that_takes_the_shape():
    want = {("xzzx", 3): "sweep", ("toric", 3): "sweep", ("rotated", 9): "sweep", ("planar", 6): "sweep", ("rotated", 11): "cut", ("planar", 7): "cut",
            ("toric", 5): "cut", ("rotated", 13): "tiled", ("xzzx", 21): "tiled", ("planar", 12): "tiled", ("toric", 7): "tiled"}
    for (code, L), route in want.items():
        got, info = ex.resolve_site_method(code, L)
        assert got == route and info["nq"] == (L * L if code in ("xzzx", "rotated") else 2 * L * L), (code, L, got)
        assert ex.resolve_method(code, L) != "tiled"                            # (exact_class_probabilities routes as it did)
    assert ex.resolve_site_method("toric", 7)[1]["held"] == 5 and ex.resolve_site_method("toric", 5)[1]["held"] == 8
    assert ex.resolve_site_method("xzzx", 3, "tiled", tile_width=4)[0] == "tiled" and ex.resolve_site_method("xzzx", 5, "cut", lds_width=6)[1]["held"] >= 1
    with pytest.raises(L_.QecmcError, match="generators wide"):
        ex.resolve_site_method("toric", 9)
    with pytest.raises(L_.QecmcError, match="generators wide"):
        ex.resolve_site_method("toric", 5, "sweep")
    with pytest.raises(L_.QecmcError, match="even length"):
        ex.resolve_site_method("toric", 4)
    with pytest.raises(L_.QecmcError, match="odd L"):
        ex.resolve_site_method("rotated", 6)
    with pytest.raises(ValueError):
        ex.resolve_site_method("xzzx", 3, "enumerate")


def test_the_builders():
    p = np.array([[0.0, 0.1], [0.25, 0.3]])
    d = ex.depolarizing_site_w4(p)
    assert d.shape == (2, 2, 4) and all(np.array_equal(d[i, j], ex.depolarizing_w4(p[i, j])) for i in range(2) for j in range(2))
    assert np.array_equal(d[0, 0], [1.0, 0.0, 0.0, 0.0])
    b = ex.biased_site_w4(p, 3.0)
    assert b.shape == (2, 2, 4) and all(np.array_equal(b[i, j], ex.biased_w4(p[i, j], 3.0)) for i in range(2) for j in range(2))
    erased = np.zeros((3, 2, 2), bool)
    erased[1, 0, 1] = erased[2, 1, 1] = True
    for base in (ex.depolarizing_w4(0.1), d):
        e = ex.erasure_site_w4(base, erased)
        assert e.shape == (3, 2, 2, 4) and e.dtype == np.float64 and e.flags.writeable
        assert np.all(e[erased] == 1.0) and np.array_equal(e[~erased], np.broadcast_to(base, e.shape)[~erased])
    assert ex.erasure_site_w4(d, erased[1]).shape == (2, 2, 4) and np.all(ex.erasure_site_w4(d, erased[1])[0, 1] == 1.0)
    rng = np.random.default_rng(5)
    m = harness.apply_erasures(np.full((4, 3, 3), 2, np.uint8), np.ones((4, 3, 3), bool), rng)
    assert set(np.unique(m).tolist()) == {0, 1, 2, 3}
    assert harness.draw_erasures("toric", 3, 50, 1.0, rng).all() and not harness.draw_erasures("toric", 3, 50, 0.0, rng).any()
    pl = harness.draw_erasures("planar", 4, 50, 1.0, rng)
    assert pl.shape == (50, 2, 4, 4) and pl[:, 0].all() and pl[:, 1, :3, :3].all() and not pl[:, 1, 3].any() and not pl[:, 1, :, 3].any()


def test_constant_rows_give_the_law_of_the_uniform_entry_points():
    """exact_site_probabilities under constant rows is exact_class_probabilities(method=...) exactly -- on a device; without one both ask for it"""
    chains = chains_of(XZZX, 5, 3)
    if L_.device_count() < 1:
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.exact_site_probabilities("xzzx", chains, np.broadcast_to(ex.depolarizing_w4(0.1), (5, 5, 4)))
        return
    for method, kw in (("sweep", {}), ("cut", dict(lds_width=6)), ("tiled", dict(tile_width=4))):
        want = ex.exact_class_probabilities("xzzx", chains, 0.1, method=method, **kw)
        assert np.array_equal(ex.exact_site_probabilities("xzzx", chains, ex.depolarizing_site_w4(np.full((5, 5), 0.1)), method=method, **kw), want)
        assert np.array_equal(ex.exact_site_probabilities("xzzx", chains, ex.depolarizing_site_w4(np.full((3, 25), 0.1)), method=method, **kw), want)


# ------------------------------------------------------------------------------------------------------ 10. the sanitizers
def test_site_sweeps_under_sanitizers():
    """a stand-alone program (its own main) built from class_sweep_site.hpp with -fsanitize=address,undefined: the three twins on weight tables
    allocated at exactly rows * nq * 4 doubles, wq_rows 1 and N, zero weights and the refusals; run as a child process"""
    run_selftest("sweep_site_asan", "class_sweep_site_selftest_asan")
