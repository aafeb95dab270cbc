"""The (min, +, count) sweep and its traceback under a cost per (syndrome, qubit) (csrc/class_minplus_site.hpp), without a GPU: the twins, compiled by
g++ into the host-table test library (qt_class_minplus_site, qt_class_minplus_chains_site), and the Python layer around them.

What is pinned: tests/util_minplus_site.py -- an elimination over the oracle's stencils with a cost row per qubit, which knows nothing of the planner
-- against a brute force at L = 3; the twins against that elimination under random byte tables and {0, 1} tables (which tie often), every traced chain
with the input's syndrome, in its class and at the site cost the sweep reports, by the oracle's functions; against the brute force at L = 3, the chain
its argmin where unique; constant rows are the uniform twins, chains included; one table is N copies of it; rows travel with their syndromes; the
planar code's unused cells are not read; pure erasure ties the twin to the site sweep's twin exactly; llr_site_costs, and the brute-force max-product
chain; refusals by code and prefix; the Python layer; the harness; the sanitizers.  Every comparison is integer or bytes and exact."""
import ctypes as C

import numpy as np
import pytest

import test_class_minplus_cpu as M
import test_class_minplus_trace_cpu as MT
import test_class_sweep_cpu as S
import test_class_sweep_cut_cpu as SC
import test_class_sweep_site_cpu as SS
import test_enumerate_cpu as E
from hostlib import run_selftest
from qecmc import _lib as L_
from qecmc import exact as ex
from qecmc import harness
from test_corrections_cpu import classes, generators, syndromes
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_minplus_site import brute_force_max_product, brute_force_minplus, eliminate_minplus, site_cost
from util_minplus_trace import coset

NAME = M.NAME
COSTS = MT.COSTS
_u8p, _u32p, _i32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
_HEAD = [C.c_int, C.c_int, C.c_uint64, _u8p, _u8p, C.c_uint64, C.c_int]


def load_twin():
    """the host-table test library with the site-cost entry points next to the uniform ones and the site sweep's (tests/test_gpu_class_minplus_site.py
    compares the GPU with it)"""
    lib = SS.load_twin()
    lib.qt_class_minplus.restype = lib.qt_class_minplus_chains.restype = C.c_int
    lib.qt_class_minplus.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _u32p, C.c_int, _u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_minplus_chains.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _u32p, C.c_int, _u8p, _u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_minplus_site.restype = lib.qt_class_minplus_chains_site.restype = C.c_int
    lib.qt_class_minplus_site.argtypes = _HEAD + [_u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_minplus_chains_site.argtypes = _HEAD + [_u8p, _u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_site_cost_words.restype = None
    lib.qt_site_cost_words.argtypes = [_u8p, C.c_uint64, C.c_int, _u32p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def nq_of(code, L):
    return int(np.prod(state_shape(code, L)))


def twin_rc(T, code, L, chains, cq, lds_width=0, rows=None, traced=True):
    """(rc, message, chains uint8[N, ncls, nq] or None, cost, count, cls) of a host twin on chains [N, ...] and cq [rows, ..., 4]; outputs start poisoned"""
    nq = nq_of(code, L) if 2 <= L <= 64 else 1
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    table = None if cq is None else np.ascontiguousarray(cq, dtype=np.uint8).reshape(-1, nq, 4)
    rows = len(table) if rows is None else rows
    ncls = 16 if code == TORIC else 4
    out = np.full((len(flat), ncls, nq), 0xEE, np.uint8)
    cost, count, cls = np.full((len(flat), ncls), 77, np.uint32), np.full((len(flat), ncls), 77, np.uint64), np.full(len(flat), 9, np.int32)
    msg = C.create_string_buffer(640)
    head = (code, L, len(flat), flat.ctypes.data_as(_u8p), None if table is None else table.ctypes.data_as(_u8p), rows, lds_width)
    tail = (cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), cls.ctypes.data_as(_i32p), msg, 640)
    if traced:
        rc = T.qt_class_minplus_chains_site(*head, out.ctypes.data_as(_u8p), *tail)
    else:
        rc = T.qt_class_minplus_site(*head, *tail)
    return rc, msg.value, out if traced else None, cost, count, cls


def twin(T, code, L, chains, cq, lds_width=0):
    """the traced twin -> (chains, cost, count, cls), with cost, count and cls checked against the sweep twin's"""
    rc, msg, out, cost, count, cls = twin_rc(T, code, L, chains, cq, lds_width)
    assert rc == 0, msg
    rc, msg, _, cost2, count2, cls2 = twin_rc(T, code, L, chains, cq, lds_width, traced=False)
    assert rc == 0, msg
    assert np.array_equal(cost, cost2) and np.array_equal(count, count2) and np.array_equal(cls, cls2)
    return out, cost, count, cls


def tables_of(code, L, rows, kind, seed=0):
    """uint8[rows, nq, 4]: "bytes": every byte value; "bits": {0, 1}, which tie often"""
    rng = np.random.default_rng([91, code, L, seed, kind == "bits"])
    return rng.integers(0, 2 if kind == "bits" else 256, size=(rows, nq_of(code, L), 4), dtype=np.uint8)


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([92, code, L, seed]))


def order_of(code, L):
    return M.toric_order(L) if code == TORIC else S.column_major(code, L) if code == PLANAR else None


def check_chains(code, L, chains, cq, out, cost):
    """every traced chain: the input's syndrome and its class by the oracle, the site cost the sweep reports"""
    gens = generators(code, L)
    table = np.asarray(cq).reshape(-1, nq_of(code, L), 4)
    assert out.max() <= 3
    syn = syndromes(code, chains)
    for s in range(len(chains)):
        got = out[s].reshape((out.shape[1],) + state_shape(code, L))
        assert np.array_equal(syndromes(code, got), np.broadcast_to(syn[s], (len(got),) + syn[s].shape)), s
        assert classes(code, got).tolist() == list(range(out.shape[1])), s
        assert [site_cost(gens, g, table[s if len(table) > 1 else 0]) for g in got] == cost[s].tolist(), s


# ------------------------------------------------------------------------------------------------------ the utility is a brute force
@pytest.mark.parametrize("code", [TORIC, PLANAR, XZZX, ROTATED])
def test_the_elimination_of_util_minplus_site_is_a_brute_force_at_L3(code):
    gens = generators(code, 3)
    for kind in ("bytes", "bits"):
        for chain, cq in zip(chains_of(code, 3, 3), tables_of(code, 3, 3, kind)):
            want = brute_force_minplus(gens, chain.ravel(), cq)
            assert eliminate_minplus(gens, chain.ravel(), cq, order_of(code, 3)) == want[:2]


# ------------------------------------------------------------------------------------------------------ the twins against the utility
SHAPES = [(ROTATED, 3, 0), (ROTATED, 5, 0), (ROTATED, 7, 0), (XZZX, 3, 0), (XZZX, 5, 0), (XZZX, 7, 0), (PLANAR, 3, 0), (PLANAR, 4, 0), (TORIC, 3, 0), (TORIC, 3, 6)]


@pytest.mark.parametrize("kind", ["bytes", "bits"])
@pytest.mark.parametrize("code,L,lds_width", SHAPES)
def test_twins_are_the_independent_elimination(T, code, L, lds_width, kind):
    n = 2
    chains, cq = chains_of(code, L, n, seed=1), tables_of(code, L, n, kind, seed=1)
    gens = generators(code, L)
    out, cost, count, cls = twin(T, code, L, chains, cq, lds_width)
    assert np.array_equal(cls, classes(code, chains))
    check_chains(code, L, chains, cq, out, cost)
    ties = 0
    for s in range(n):
        want = [eliminate_minplus(gens, np.asarray(r).ravel(), cq[s], order_of(code, L)) for r in E.class_chains(code, chains[s])]
        assert all(c % (1 << M.shift_of(code)) == 0 for _, c in want)
        assert [(int(a), int(b) << M.shift_of(code)) for a, b in zip(cost[s], count[s])] == want, (s, want)
        ties += sum(c >> M.shift_of(code) > 1 for _, c in want)
    print(NAME[code], L, lds_width, kind, "classes with tied shortest chains:", ties)
    if kind == "bits" and L >= 5:
        assert ties >= 1


@pytest.mark.parametrize("kind", ["bytes", "bits"])
@pytest.mark.parametrize("code", [TORIC, PLANAR, XZZX, ROTATED])
def test_twins_are_a_brute_force_at_L3_and_unique_chains_its_argmin(T, code, kind):
    gens = generators(code, 3)
    n = 2 if code == TORIC else 6
    chains, cq = chains_of(code, 3, n, seed=2), tables_of(code, 3, n, kind, seed=2)
    out, cost, count, cls = twin(T, code, 3, chains, cq)
    unique = 0
    for s in range(n):
        for c, rep in enumerate(E.class_chains(code, chains[s])):
            least, subsets, best = brute_force_minplus(gens, np.asarray(rep).ravel(), cq[s])
            assert (int(cost[s, c]), int(count[s, c])) == (least, subsets >> M.shift_of(code)) and len(best) == int(count[s, c])
            assert any(np.array_equal(out[s, c], b) for b in best)              # tied or not, it is one of the shortest
            if count[s, c] == 1:
                assert np.array_equal(out[s, c], best[0])
                unique += 1
    print(NAME[code], kind, "unique rows compared with the brute force:", unique)
    assert unique >= (4 if kind == "bytes" else 0)


# ------------------------------------------------------------------------------------------------------ constant rows, one table, permutations
@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 5, 0), (XZZX, 5, 6), (PLANAR, 4, 0), (TORIC, 3, 0), (TORIC, 3, 6)])
def test_constant_rows_are_the_uniform_twins_chains_included(T, code, L, lds_width, costs):
    chains = chains_of(code, L, 4, seed=3)
    cq = np.broadcast_to(np.array(costs, np.uint8), (1, nq_of(code, L), 4))
    out, cost, count, cls = twin(T, code, L, chains, cq, lds_width)
    want = MT.twin(T, code, L, chains, costs, lds_width)
    for got, ref in zip((out, cost, count, cls), want):
        assert np.array_equal(got, ref)
    rows = np.broadcast_to(cq, (4, nq_of(code, L), 4))
    for got, ref in zip(twin(T, code, L, chains, rows, lds_width), want):
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 5, 0), (PLANAR, 3, 0), (TORIC, 3, 6)])
def test_one_table_is_n_copies_of_it_and_rows_travel_with_their_syndromes(T, code, L, lds_width):
    n = 5
    chains = chains_of(code, L, n, seed=4)
    one = tables_of(code, L, 1, "bytes", seed=4)
    a, b = twin(T, code, L, chains, one, lds_width), twin(T, code, L, chains, np.repeat(one, n, axis=0), lds_width)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    cq = tables_of(code, L, n, "bytes", seed=5)
    base = twin(T, code, L, chains, cq, lds_width)
    perm = np.random.default_rng(6).permutation(n)
    moved = twin(T, code, L, chains[perm], cq[perm], lds_width)
    assert all(np.array_equal(x[perm], y) for x, y in zip(base, moved))
    wrong = twin(T, code, L, chains[perm], cq, lds_width)                       # (the rows matter: left in place they give other costs)
    assert not np.array_equal(wrong[1], moved[1])
    for s in range(n):                                                          # row s alone, as the one table of syndrome s
        alone = twin(T, code, L, chains[s:s + 1], cq[s:s + 1], lds_width)
        assert all(np.array_equal(x[s:s + 1], y) for x, y in zip(base, alone))


def test_the_planar_codes_unused_cells_are_not_read(T):
    for L, lds_width in ((3, 0), (4, 0), (3, 3)):
        chains = chains_of(PLANAR, L, 3, seed=7)
        cq = tables_of(PLANAR, L, 3, "bytes", seed=7).reshape(3, 2, L, L, 4)
        want = twin(T, PLANAR, L, chains, cq, lds_width)
        for fill in (0, 255):
            dirty = cq.copy()
            dirty[:, 1, -1, :] = fill
            dirty[:, 1, :, -1] = fill
            assert not np.array_equal(dirty, cq)
            assert all(np.array_equal(x, y) for x, y in zip(twin(T, PLANAR, L, chains, dirty, lds_width), want))
        dirty = cq.copy()
        dirty[:, 0, 0, 0] ^= 0x55                                               # a qubit: the costs move
        assert not np.array_equal(twin(T, PLANAR, L, chains, dirty, lds_width)[1], want[1])


def test_the_cost_words_are_in_xz_order(T):
    cq = np.array([[[1, 2, 3, 4], [0, 255, 7, 9]]], np.uint8)
    words = np.zeros(2, np.uint32)
    T.qt_site_cost_words(cq.ctypes.data_as(_u8p), 1, 2, words.ctypes.data_as(_u32p))
    assert words.tolist() == [0x03040201, 0x0709FF00]                           # bytes I, X, Z, Y from the lowest


# ------------------------------------------------------------------------------------------------------ pure erasure
ERASURE_SHAPES = [(ROTATED, 5), (XZZX, 5), (PLANAR, 4), (TORIC, 3)]
_erasure = {}


def erasure_case(code, L, n=8):
    """n shots of the pure-erasure channel, computed once: shot 0 has row 1 and column 1 of every layer erased, the others random sets; every set has at
    most 20 qubits, so a class holds fewer than 4^20 = 2^40 chains.  dict(erased bool[n, ...], chains: uniform Paulis on the erased cells -- an error
    with the shot's syndrome --, cq: erasure_site_costs of unit costs, wq: erasure_site_w4 of (1, 0, 0, 0))"""
    if (code, L) not in _erasure:
        rng = np.random.default_rng([93, code, L])
        cells = harness._qubit_cells(code, L)
        erased = np.zeros((n,) + cells.shape, bool)
        erased[0, ..., 1, :] = True
        erased[0, ..., :, 1] = True
        erased[1:] = rng.random((n - 1,) + cells.shape) < 0.3
        erased &= cells
        assert erased.reshape(n, -1).sum(axis=1).max() <= 20 and erased.reshape(n, -1).sum(axis=1).min() >= 1
        chains = harness.apply_erasures(np.zeros((n,) + cells.shape, np.uint8), erased, rng)
        _erasure[code, L] = dict(erased=erased, chains=chains, cq=ex.erasure_site_costs((0, 1, 1, 1), erased),
                                 wq=ex.erasure_site_w4(np.array([1.0, 0.0, 0.0, 0.0]), erased))
    return _erasure[code, L]


def check_pure_erasure(z, cost, count, ranked):
    """Z of the site sweep under (1, 0, 0, 0) off the erased set counts the chains inside it: exactly the count of the classes at cost 0"""
    assert count.max() < 1 << 46 and count.min() >= 1
    want = np.where(cost == 0, count, 0)
    assert np.array_equal(z, want.astype(np.float64)) and np.array_equal(z.astype(np.uint64), want)
    assert (cost == 0).any(axis=1).all()                                        # the error itself lies in the erased set
    assert ((cost == 0).sum(axis=1) > 1).any()                                  # a logical operator fits into some shot's erased set
    assert np.array_equal(ranked, np.argmax(z, axis=1))                          # both break ties towards the lower class index: no row is excluded


@pytest.mark.parametrize("code,L", ERASURE_SHAPES)
def test_pure_erasure_ties_the_twin_to_the_site_sweeps_twin(T, code, L):
    case = erasure_case(code, L)
    assert case["cq"].dtype == np.uint8 and case["cq"].shape == case["erased"].shape + (4,)
    assert not case["cq"][case["erased"]].any() and np.all(case["cq"][~case["erased"]] == [0, 1, 1, 1])
    out, cost, count, cls = twin(T, code, L, case["chains"], case["cq"])
    z, _ = SS.twin(T, "cut", code, L, case["chains"], case["wq"], (0,))
    check_pure_erasure(z, cost, count, ex._rank_classes(cost, count))
    assert np.all(cost[np.arange(len(cls)), cls] == 0)
    check_chains(code, L, case["chains"], case["cq"], out, cost)


# ------------------------------------------------------------------------------------------------------ log-likelihood costs
def test_llr_site_costs_of_exact_powers_are_the_exponents():
    rng = np.random.default_rng(94)
    for base in (0.5, 0.1, 1e-3, 0.9):
        k = rng.integers(0, 40, size=(3, 7, 4))
        k[..., 0] = 0                                                           # (the identity is the likeliest: the exponents are the costs themselves)
        got = ex.llr_site_costs(np.power(base, k), 1.0 / np.log(1.0 / base))
        assert got.dtype == np.uint8 and np.array_equal(got, k)
    k = np.array([[3, 1, 4, 2]])                                                # the likeliest Pauli costs 0 wherever it sits
    assert ex.llr_site_costs(np.power(0.5, k), 1.0 / np.log(2.0)).tolist() == [[2, 0, 3, 1]]
    assert ex.llr_site_costs(np.ones((2, 4)), 7.0).tolist() == [[0] * 4] * 2
    with pytest.raises(ValueError, match=r"site_w4\[1\]\[Y\]=0.0"):
        ex.llr_site_costs(np.array([[1, 1, 1, 1], [1, 0.5, 0, 1.0]]), 1.0)
    with pytest.raises(ValueError, match=r"site_w4\[0, 2\]\[Z\]=(nan|inf)"):
        ex.llr_site_costs(np.array([[[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, np.inf]]]), 1.0)
    with pytest.raises(ValueError, match=r"site_w4\[0\]\[X\]=-1.0"):
        ex.llr_site_costs(np.array([[1, -1.0, 1, 1]]), 1.0)
    with pytest.raises(ValueError, match=r"site_w4\[0\]\[Z\]: a cost of 256 .* passes 255"):
        ex.llr_site_costs(np.power(0.5, np.array([[0, 1, 255, 256]])), 1.0 / np.log(2.0))
    assert ex.llr_site_costs(np.power(0.5, np.array([[0, 1, 254, 255]])), 1.0 / np.log(2.0)).tolist() == [[0, 1, 254, 255]]
    with pytest.raises(ValueError, match="site_w4 of shape"):
        ex.llr_site_costs(np.ones((3, 3)), 1.0)


@pytest.mark.parametrize("code", [TORIC, PLANAR, XZZX, ROTATED])
def test_the_most_likely_chain_of_a_class_at_L3(T, code):
    """weights that are powers of 1 / 2 -- products are exact in float64 --: where one chain of the class has the largest product, it is the traced chain
    under llr_site_costs"""
    gens = generators(code, 3)
    n = 2 if code == TORIC else 5
    rng = np.random.default_rng([95, code])
    k = rng.integers(0, 6, size=(n, nq_of(code, 3), 4))
    wq = np.power(0.5, k)
    cq = ex.llr_site_costs(wq, 1.0 / np.log(2.0))
    assert np.array_equal(cq, k - k.min(axis=-1, keepdims=True))
    chains = chains_of(code, 3, n, seed=8)
    out, cost, count, cls = twin(T, code, 3, chains, cq)
    unique = 0
    for s in range(n):
        for c, rep in enumerate(E.class_chains(code, chains[s])):
            best = brute_force_max_product(gens, np.asarray(rep).ravel(), wq[s])
            assert len(best) == int(count[s, c])
            assert any(np.array_equal(out[s, c], b) for b in best)
            if len(best) == 1:
                assert np.array_equal(out[s, c], best[0])
                unique += 1
    print(NAME[code], "classes with one most likely chain:", unique)
    assert unique >= 4


# ------------------------------------------------------------------------------------------------------ refusals
PLAN_REFUSED = [r for r in M.REFUSED if r[2] == M.UNIT]                         # (what the plan refuses; a byte cannot pass 255)


@pytest.mark.parametrize("traced,prefix", [(False, b"qecmc_class_minplus_site:"), (True, b"qecmc_class_minplus_chains_site:")])
def test_refusals_by_code_and_prefix(T, traced, prefix):
    assert len(PLAN_REFUSED) >= 6
    for code, L, _, w, want, frags in PLAN_REFUSED:
        nq = nq_of(code, L)
        rc, msg, out, cost, _, _ = twin_rc(T, code, L, np.zeros((1, nq), np.uint8), np.zeros((1, nq, 4), np.uint8), w, traced=traced)
        print(NAME[code], L, w, msg)
        assert rc == want and msg.startswith(prefix) and all(f in msg for f in frags), (code, L, w, msg)
        assert np.all(cost == 77) and (out is None or np.all(out == 0xEE))
    chains, cq = np.zeros((3, 9), np.uint8), np.zeros((3, 9, 4), np.uint8)
    rc, msg, _, _, _, _ = twin_rc(T, ROTATED, 3, chains, None, traced=traced, rows=1)
    assert rc == -1 and msg.startswith(prefix) and b"NULL" in msg
    for rows in (0, 2, 4):
        rc, msg, _, cost, _, _ = twin_rc(T, ROTATED, 3, chains, cq, traced=traced, rows=rows)
        assert rc == -1 and msg.startswith(prefix) and b"cq_rows=%d" % rows in msg and b"one table (1) or one per syndrome (N=3)" in msg, msg
        assert np.all(cost == 77)
    for rows in (1, 3):
        assert twin_rc(T, ROTATED, 3, chains, cq, traced=traced, rows=rows)[0] == 0
    assert twin_rc(T, ROTATED, 3, chains[:0], cq, traced=traced, rows=7)[0] == 0  # N == 0: any rows
    assert twin_rc(T, ROTATED, 3, chains, np.full((3, 9, 4), 255, np.uint8), traced=traced)[0] == 0         # every byte is a cost


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    assert lib.qecmc_abi_version() == 4
    big = np.zeros((1, 2 * 13 * 13), np.uint8)
    cq = np.zeros((1, 2 * 13 * 13, 4), np.uint8)
    out = np.zeros((1, 16, 2 * 13 * 13), np.uint8)
    cost, count, cls = np.zeros((1, 16), np.uint32), np.zeros((1, 16), np.uint64), np.zeros(1, np.int32)
    tail = (cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), L_.i32(cls))
    sweep = lambda code, L, w, n=1, rows=1, table=cq: lib.qecmc_class_minplus_site(code, L, n, L_.u8(big), None if table is None else L_.u8(table), rows, w, *tail)
    trace = lambda code, L, w, n=1, rows=1, table=cq: lib.qecmc_class_minplus_chains_site(code, L, n, L_.u8(big), None if table is None else L_.u8(table), rows, w,
                                                                                           L_.u8(out), *tail)
    for call, prefix in ((sweep, b"qecmc_class_minplus_site:"), (trace, b"qecmc_class_minplus_chains_site:")):
        for code, L, _, w, want, frags in PLAN_REFUSED:
            assert call(code, L, w) == want
            err = lib.qecmc_last_error()
            assert err.startswith(prefix) and all(f in err for f in frags), err
        assert call(ROTATED, 3, 0, table=None) == -1 and lib.qecmc_last_error().startswith(prefix) and b"NULL" in lib.qecmc_last_error()
        assert call(ROTATED, 3, 0, n=1, rows=2) == -1 and lib.qecmc_last_error().startswith(prefix + b" cq_rows=2")
        have = L_.device_count() >= 1
        for n in (1, 0):
            assert call(ROTATED, 3, 0, n=n) == (0 if have else -2)
        if not have:
            assert b"no CPU fallback" in lib.qecmc_last_error()
    assert lib.qecmc_class_minplus_chains_site(ROTATED, 3, 1, L_.u8(big), L_.u8(cq), 1, 0, None, None, None, None) == -1
    assert lib.qecmc_class_minplus_site(ROTATED, 3, 1, L_.u8(big), L_.u8(cq), 1, 0, None, tail[1], None) == -1


# ------------------------------------------------------------------------------------------------------ the Python layer
class _TwinLibrary:
    """the library with the four min-plus entry points answered by the host twins: what the Python layer does around the calls needs no device"""

    def __init__(self, real, T):
        self._real, self._T = real, T

    def __getattr__(self, name):
        return getattr(self._real, name)

    def qecmc_class_minplus(self, *args):
        return self._T.qt_class_minplus(*args, None, 0)

    def qecmc_class_minplus_chains(self, *args):
        return self._T.qt_class_minplus_chains(*args, None, 0)

    def qecmc_class_minplus_site(self, *args):
        return self._T.qt_class_minplus_site(*args, None, 0)

    def qecmc_class_minplus_chains_site(self, *args):
        return self._T.qt_class_minplus_chains_site(*args, None, 0)


def test_python_layer_shapes_keys_and_rankings(T, monkeypatch):
    import qecmc
    for name in ("class_minplus_site", "shortest_chains_site", "min_weight_classes_site", "min_weight_corrections_site", "erasure_site_costs", "llr_site_costs"):
        assert getattr(qecmc, name) is getattr(ex, name) and name in qecmc.__all__
    real = L_.lib()
    monkeypatch.setattr(ex.L_, "lib", lambda: _TwinLibrary(real, T))
    for code, L, lds_width in [(ROTATED, 5, 0), (TORIC, 3, 6), (PLANAR, 3, 0)]:
        n, nq, ncls = 5, nq_of(code, L), 16 if code == TORIC else 4
        chains = chains_of(code, L, n, seed=9)
        cq = tables_of(code, L, n, "bytes", seed=9)
        out, cost, count, cls = twin(T, code, L, chains, cq, lds_width)
        r = ex.shortest_chains_site(NAME[code], chains, cq.reshape((n,) + state_shape(code, L) + (4,)), lds_width=lds_width)
        m = ex.class_minplus_site(NAME[code], chains, cq, lds_width=lds_width)
        assert set(r) == set(ex.shortest_chains(NAME[code], chains, lds_width=lds_width)) and set(m) == set(ex.class_minplus(NAME[code], chains, lds_width=lds_width))
        assert r["chains"].shape == (n, ncls) + state_shape(code, L) and r["chains"].dtype == np.uint8
        assert np.array_equal(r["chains"].reshape(out.shape), out)
        for d in (r, m):
            assert np.array_equal(d["cost"], cost) and np.array_equal(d["count"], count) and np.array_equal(d["cls"], cls)
            assert np.array_equal(d["saturated"], count == 0)
            inf = SC.info(T, code, L, lds_width)[1]
            assert (d["width"], d["held"]) == (inf["width"], inf["held"])
        assert np.array_equal(r["unique"], count == 1)
        # one table: the matrix shape, the flat shape, a leading 1 -- and the flat chains with size=
        one = ex.class_minplus_site(code, chains.reshape(n, -1), cq[0], size=L, lds_width=lds_width)
        for table in (cq[0].reshape(state_shape(code, L) + (4,)), cq[:1], cq[:1].reshape((1,) + state_shape(code, L) + (4,)), cq[0].astype(np.int64), cq[0].astype(float)):
            again = ex.class_minplus_site(NAME[code], chains, table, lds_width=lds_width)
            assert np.array_equal(again["cost"], one["cost"]) and np.array_equal(again["count"], one["count"])
        assert np.array_equal(one["cost"], twin(T, code, L, chains, cq[:1], lds_width)[1])
        target = ex._rank_classes(cost, count)
        assert np.array_equal(ex.min_weight_classes_site(NAME[code], chains, cq, lds_width=lds_width), target)
        c = ex.min_weight_corrections_site(NAME[code], chains, cq, lds_width=lds_width)
        assert np.array_equal(c["target"], target) and c["correction"].shape == chains.shape
        assert np.array_equal(c["correction"], r["chains"][np.arange(n), target])
        assert np.array_equal(c["weight"], cost.min(axis=1)) and c["weight"].dtype == np.uint32
        # shortest_class_law under a table: count * base^cost, and with constant rows the uniform law
        law = ex.shortest_class_law(NAME[code], chains, 0.05, site_costs=cq, lds_width=lds_width)
        assert np.array_equal(law, ex._law_from_minplus(cost, count, count == 0, (0.05 / 3.0) / 0.95))
        const = np.broadcast_to(np.array([0, 3, 3, 1], np.uint8), (nq, 4))
        assert np.array_equal(ex.shortest_class_law(NAME[code], chains, 0.2, alpha=3, site_costs=const, lds_width=lds_width),
                              ex.shortest_class_law(NAME[code], chains, 0.2, alpha=3, lds_width=lds_width))


def test_python_checks_its_arguments_before_the_library():
    chains = np.zeros((2, 3, 3), np.uint8)
    good = np.zeros((3, 3, 4), np.int64)
    for bad, cell in [(1.5, r"site_costs\[row 0\]\[qubit 4\]\[Y\]=1.5"), (-1, r"site_costs\[row 0\]\[qubit 4\]\[Y\]=-1.0"), (256, r"site_costs\[row 0\]\[qubit 4\]\[Y\]=256.0"),
                      (np.nan, r"site_costs\[row 0\]\[qubit 4\]\[Y\]=nan")]:
        table = good.astype(float)
        table[1, 1, 2] = bad
        table[2, 2, 3] = bad                                                    # the first offending cell is named
        for fn in (ex.class_minplus_site, ex.shortest_chains_site, ex.min_weight_classes_site, ex.min_weight_corrections_site):
            with pytest.raises(ValueError, match=cell + ".*integers 0 .. 255"):
                fn("rotated", chains, table)
    rows = np.zeros((2, 9, 4))
    rows[1, 8, 0] = 300
    with pytest.raises(ValueError, match=r"site_costs\[row 1\]\[qubit 8\]\[I\]=300.0"):
        ex.class_minplus_site("rotated", chains, rows)
    for shape in [(3, 3), (3, 3, 3), (3, 9, 4), (2, 3, 3, 5), (4,)]:
        with pytest.raises(ValueError, match="site_costs of shape"):
            ex.class_minplus_site("rotated", chains, np.zeros(shape, np.uint8))
    with pytest.raises(ValueError, match="site_costs of dtype"):
        ex.class_minplus_site("rotated", chains, np.zeros((3, 3, 4), complex))
    with pytest.raises(ValueError, match="base_costs"):
        ex.erasure_site_costs((0, 1, 1, 256), np.zeros((3, 3), bool))
    with pytest.raises(ValueError, match="base_costs"):
        ex.erasure_site_costs((0, 0.5, 1, 1), np.zeros((3, 3), bool))
    e = ex.erasure_site_costs(np.arange(36).reshape(3, 3, 4), np.eye(3, dtype=bool))
    assert e.dtype == np.uint8 and e.shape == (3, 3, 4) and not e[np.eye(3, dtype=bool)].any() and e[0, 1].tolist() == [4, 5, 6, 7]


def test_harness_refuses_site_costs_under_another_method_and_biased_erasures():
    cq = np.zeros((5, 5, 4), np.uint8)
    for method in ("PTEQ", "exact", "STDC"):
        with pytest.raises(ValueError, match="params\\['site_costs'\\] is built for method min_weight, not " + method):
            harness.generate(dict(code="rotated", size=5, p_error=0.1, method=method, site_costs=cq), 4)
    with pytest.raises(ValueError, match="params\\['site_costs'\\] is built for method min_weight, not exact"):
        harness.decode_syndromes(dict(code="rotated", size=5, p_error=0.1, method="exact", site_costs=cq), np.zeros((1, 36), np.uint8))
    with pytest.raises(ValueError, match="params\\['site_costs'\\] is built for method min_weight, not PTEQ"):
        harness.threshold_curve(dict(code="rotated", size=5, noise="depolarizing", site_costs=cq), [0.1], 4)
    params = dict(code="rotated", size=5, p_error=0.1, p_erase=0.1, noise="biased", eta=10.0)
    with pytest.raises(ValueError, match="method min_weight is defined for depolarizing and alpha noise, not biased"):
        harness.erasure_experiment(params, 4, method="min_weight")
    with pytest.raises(ValueError, match="alpha=2.5"):
        harness.erasure_experiment(dict(params, noise="alpha", alpha=2.5), 4, method="min_weight")
    with pytest.raises(ValueError, match="method='PTEQ'"):
        harness.erasure_experiment(params, 4, method="PTEQ")


# ------------------------------------------------------------------------------------------------------ the sanitizers
def test_minplus_site_under_sanitizers():
    """a stand-alone program (its own main) built from class_minplus_site.hpp with -fsanitize=address,undefined: the site plans against the uniform
    plans, the twins over cost tables, scratch, decision words and outputs allocated at their exact size; run as a child process"""
    run_selftest("minplus_site_asan", "class_minplus_site_selftest_asan")
