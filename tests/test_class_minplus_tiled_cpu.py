"""The (min, +, count) sweep on the tiled plans (csrc/class_minplus_tiled.hpp), without a GPU: the twins minplus_tiled_host and
minplus_tiled_site_host, compiled by g++ into the host-table test library (qt_class_minplus_tiled, qt_class_minplus_tiled_site), and the Python layer
around them.

What is pinned: the twin against minplus_cut_host exactly where both take the shape; against tests/util_minplus.eliminate_minplus -- which knows
nothing of the planner -- at rotated L = 13 and planar L = 8, the first shapes only this route takes, under three cost vectors; forced holds against
the plan with none; a sector law for (min, +) (tests/util_minplus_sectors.py) against a brute force at L = 3 and against the twin at rotated / xzzx
L = 13 and 15, where a CLOSE names a fixed slot >= 16; the site twin with constant rows, a row per syndrome and the planar code's unused cells
poisoned; the cost-range refusals, the tiled plan's refusals under this entry point's name, the ABI version, N == 0; the Python layer and the
harness.  Every comparison is of integers and exact."""
import ctypes as C

import numpy as np
import pytest

import test_class_minplus_cpu as M
import test_class_minplus_site_cpu as MS
import test_class_sweep_tiled_cpu as ST
import test_enumerate_cpu as E
from qecmc import _lib as L_
from qecmc import exact as ex
from qecmc import harness
from test_corrections_cpu import classes, generators
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_minplus import brute_force_minplus, eliminate_minplus
from util_minplus_sectors import sector_minplus
from util_sectors import bit_rows, gf2_rank, order_for, sectors

NAME = M.NAME
UNIT, SPLIT, SPLIT2 = (0, 1, 1, 1), (0, 1, 2, 1), (0, 2, 2, 1)                  # SPLIT: c_Y = c_X + c_Z, the sector law's costs
COSTS = [UNIT, SPLIT, SPLIT2]
_u8p, _u32p, _i32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
PREFIX, SITE_PREFIX = b"qecmc_class_minplus_tiled:", b"qecmc_class_minplus_tiled_site:"


def load_twin():
    """the host-table test library with the tiled min-plus entry points next to every sibling's (tests/test_gpu_class_minplus_tiled.py compares the GPU
    with it)"""
    lib = MS.load_twin()
    lib.qt_class_minplus_tiled.restype = lib.qt_class_minplus_tiled_site.restype = C.c_int
    lib.qt_class_minplus_tiled.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _u32p, C.c_int, C.c_int, _u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_minplus_tiled_site.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _u8p, C.c_uint64, C.c_int, C.c_int, _u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def nq_of(code, L):
    return int(np.prod(state_shape(code, L))) if 2 <= L <= 64 and code in (TORIC, PLANAR, XZZX, ROTATED) else 1


def twin_rc(T, code, L, chains, costs, hbm_width=0, tile_width=0):
    """(rc, message, cost uint32[N, ncls], count uint64[N, ncls], cls int32[N]) of the uniform twin on chains [N, ...]; outputs start poisoned"""
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq_of(code, L))
    c = np.array(costs, np.uint32)
    ncls = 16 if code == TORIC else 4
    cost, count, cls = np.full((len(flat), ncls), 77, np.uint32), np.full((len(flat), ncls), 77, np.uint64), np.full(len(flat), 9, np.int32)
    msg = C.create_string_buffer(640)
    rc = T.qt_class_minplus_tiled(code, L, len(flat), flat.ctypes.data_as(_u8p), c.ctypes.data_as(_u32p), hbm_width, tile_width, cost.ctypes.data_as(_u32p),
                                  count.ctypes.data_as(_u64p), cls.ctypes.data_as(_i32p), msg, 640)
    return rc, msg.value, cost, count, cls


def twin(T, code, L, chains, costs, hbm_width=0, tile_width=0):
    rc, msg, cost, count, cls = twin_rc(T, code, L, chains, costs, hbm_width, tile_width)
    assert rc == 0, msg
    return cost, count, cls


def site_twin_rc(T, code, L, chains, cq, hbm_width=0, tile_width=0, rows=None):
    """the site twin on chains [N, ...] and cq [rows, ..., 4]"""
    nq = nq_of(code, L)
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    table = None if cq is None else np.ascontiguousarray(cq, dtype=np.uint8).reshape(-1, nq, 4)
    rows = len(table) if rows is None else rows
    ncls = 16 if code == TORIC else 4
    cost, count, cls = np.full((len(flat), ncls), 77, np.uint32), np.full((len(flat), ncls), 77, np.uint64), np.full(len(flat), 9, np.int32)
    msg = C.create_string_buffer(640)
    rc = T.qt_class_minplus_tiled_site(code, L, len(flat), flat.ctypes.data_as(_u8p), None if table is None else table.ctypes.data_as(_u8p), rows, hbm_width, tile_width,
                                       cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), cls.ctypes.data_as(_i32p), msg, 640)
    return rc, msg.value, cost, count, cls


def site_twin(T, code, L, chains, cq, hbm_width=0, tile_width=0):
    rc, msg, cost, count, cls = site_twin_rc(T, code, L, chains, cq, hbm_width, tile_width)
    assert rc == 0, msg
    return cost, count, cls


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([61, code, L, seed]))


def few_errors(code, L, n, k, seed=0):
    """n chains with k errors each at cells that hold a qubit: few enough that every class keeps few shortest chains (the GPU tests' top shapes)"""
    rng = np.random.default_rng([62, code, L, seed])
    cells = np.flatnonzero(harness._qubit_cells(code, L).ravel())
    out = np.zeros((n, nq_of(code, L)), np.uint8)
    for row in out:
        row[rng.choice(cells, size=k, replace=False)] = rng.integers(1, 4, size=k, dtype=np.uint8)
    return out.reshape((n,) + state_shape(code, L))


_tables = {}


def sector_law(code, L, chains, costs):
    """(cost int64[N, ncls], count object[N, ncls]) by the sector law: every class of every chain through the oracle's logical operators"""
    if (code, L) not in _tables:
        gens = generators(code, L)
        _tables[code, L] = gens, sectors(gens), gf2_rank(bit_rows(gens))
    gens, parts, rank = _tables[code, L]
    rows = [[sector_minplus(gens, np.asarray(r).ravel(), costs, order_for(code, L), parts, rank) for r in E.class_chains(code, c)] for c in chains]
    return np.array([[a for a, _ in r] for r in rows], np.int64), np.array([[b for _, b in r] for r in rows], dtype=object)


def same_as_law(cost, count, want_cost, want_count, limit=1 << 48):
    """the sweep's (cost, count) against Python integers: equal where the law's count stays below the saturation limit, which the caller's chains see to"""
    assert np.array_equal(cost.astype(np.int64), want_cost), (cost, want_cost)
    assert all(int(c) < limit for c in want_count.ravel()), want_count
    assert [int(c) for c in count.ravel()] == [int(c) for c in want_count.ravel()]


# ------------------------------------------------------------------------------------------------------ the twin against the cut twin
@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("code,L,hbm_width,lds_width", [(TORIC, 3, 13, 13), (ROTATED, 7, 0, 0), (ROTATED, 9, 0, 0), (PLANAR, 5, 0, 0)])
def test_twin_is_the_cut_twin_where_both_take_the_shape(T, code, L, hbm_width, lds_width, costs):
    chains = chains_of(code, L, 3)
    want = M.twin(T, code, L, chains, costs, lds_width)
    got = twin(T, code, L, chains, costs, hbm_width)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(got[2], classes(code, chains)) and got[1].min() >= 1


# ------------------------------------------------------------------------------------------------------ ... and an independent elimination
_first = {}


def first_shapes_case(T, code, L, costs):
    """two chains at a shape only the tiled route takes, and the twin under one cost vector, computed once (tests/test_gpu_class_minplus_tiled.py reads
    the rotated L = 13 rows)"""
    key = (code, L, tuple(costs))
    if key not in _first:
        chains = chains_of(code, L, 2, seed=1)
        _first[key] = (chains,) + twin(T, code, L, chains, costs)
    return _first[key]


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("code,L", [(ROTATED, 13), (PLANAR, 8)])
def test_twin_is_the_independent_elimination_at_the_first_tiled_shapes(T, code, L, costs):
    chains, cost, count, cls = first_shapes_case(T, code, L, costs)
    assert ST.info(T, code, L)[1]["width"] == 16 and M.twin_rc(T, code, L, chains, costs)[0] == -4     # (the cut plans refuse the shape)
    gens = generators(code, L)
    assert np.array_equal(cls, classes(code, chains))
    for s in range(len(chains)):
        want = [eliminate_minplus(gens, np.asarray(r).ravel(), costs, order_for(code, L), max_axes=17) for r in E.class_chains(code, chains[s])]
        assert [(int(a), int(b)) for a, b in zip(cost[s], count[s])] == want, (s, want)


# ------------------------------------------------------------------------------------------------------ forced holds, tile widths
@pytest.mark.parametrize("costs", COSTS)
def test_forced_holds_equal_the_plan_with_none(T, costs):
    inf = ST.info(T, TORIC, 3, 8, 4)[1]
    assert inf["held"] >= 1 and inf["width"] <= 8 and ST.info(T, TORIC, 3)[1]["held"] == 0
    chains = chains_of(TORIC, 3, 4, seed=2)
    want = twin(T, TORIC, 3, chains, costs)
    for a, b in zip(twin(T, TORIC, 3, chains, costs, 8, 4), want):
        assert np.array_equal(a, b)
    for a, b in zip(twin(T, TORIC, 3, chains, costs, 0, 6), want):              # (the tile width is no part of the host loop: the plan's ops are)
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------ the sector law
@pytest.mark.parametrize("code", [TORIC, PLANAR, XZZX, ROTATED])
def test_the_sector_law_is_a_brute_force_at_L3(code):
    gens = generators(code, 3)
    shift = len(gens) - gf2_rank(bit_rows(gens))
    assert shift == M.shift_of(code)
    for costs in (SPLIT, (0, 3, 5, 2), (0, 0, 1, 1)):
        for chain in chains_of(code, 3, 3, seed=3):
            for rep in E.class_chains(code, chain):
                least, subsets = brute_force_minplus(gens, np.asarray(rep).ravel(), costs)
                assert sector_minplus(gens, np.asarray(rep).ravel(), costs, order_for(code, 3)) == (least, subsets >> shift)
    with pytest.raises(AssertionError, match="c_Y = c_X \\+ c_Z"):
        sector_minplus(gens, np.zeros(gens.shape[1], np.uint8), UNIT)


def fixed_slots_closed(T, code, L):
    """the highest fixed slot (outside its segment's tile) some CLOSE of the default plan names"""
    ops, top = ST.ops_of(T, code, L), -1
    for sg in ST.segments_of(T, code, L):
        for kind, _, _, _, pairs, _ in ops[sg["op_first"]:sg["op_first"] + sg["op_count"]]:
            if kind == ST.CLOSE:
                top = max([top] + [s for s, _ in pairs if not (sg["tile"] >> s) & 1])
    return top


@pytest.mark.parametrize("code,L", [(ROTATED, 13), (XZZX, 13), (ROTATED, 15), (XZZX, 15)])
def test_twin_is_the_sector_law_at_L13_and_L15(T, code, L):
    """one chain each under costs (0, 1, 2, 1); at L = 15 the state vector is 18 wide and a CLOSE names a fixed slot >= 16"""
    assert fixed_slots_closed(T, code, L) >= (16 if L == 15 else 11)
    chains = few_errors(code, L, 1, 12, seed=L)
    cost, count, cls = twin(T, code, L, chains, SPLIT)
    same_as_law(cost, count, *sector_law(code, L, chains, SPLIT))
    assert np.array_equal(cls, classes(code, chains)) and cost[0, cls[0]] <= 24 and len(set(cost[0].tolist())) > 1


# ------------------------------------------------------------------------------------------------------ the site twin
@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4), (PLANAR, 5, 0, 0)])
def test_site_twin_constant_rows_and_a_row_per_syndrome(T, code, L, hbm_width, tile_width):
    n, nq = 4, nq_of(code, L)
    chains = chains_of(code, L, n, seed=4)
    for costs in COSTS + [(1, 0, 2, 3)]:
        want = twin(T, code, L, chains, costs, hbm_width, tile_width)
        for rows in (1, n):
            cq = np.broadcast_to(np.array(costs, np.uint8), (rows, nq, 4))
            for a, b in zip(site_twin(T, code, L, chains, cq, hbm_width, tile_width), want):
                assert np.array_equal(a, b)
    cq = MS.tables_of(code, L, n, "bytes", seed=4)
    base = site_twin(T, code, L, chains, cq, hbm_width, tile_width)
    if hbm_width in (0, 13):
        rc, msg, _, cost, count, cls = MS.twin_rc(T, code, L, chains, cq, hbm_width, traced=False)      # the cut site twin takes these shapes too
        assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(base, (cost, count, cls))), msg
    for s in range(n):                                                          # row s alone, as the one table of syndrome s
        alone = site_twin(T, code, L, chains[s:s + 1], cq[s:s + 1], hbm_width, tile_width)
        assert all(np.array_equal(x[s:s + 1], y) for x, y in zip(base, alone))
    perm = np.random.default_rng(5).permutation(n)
    moved = site_twin(T, code, L, chains[perm], cq[perm], hbm_width, tile_width)
    assert all(np.array_equal(x[perm], y) for x, y in zip(base, moved))
    assert not np.array_equal(site_twin(T, code, L, chains[perm], cq, hbm_width, tile_width)[0], moved[0])


def test_site_twin_does_not_read_the_planar_codes_unused_cells(T):
    L = 5
    chains = chains_of(PLANAR, L, 3, seed=6)
    cq = MS.tables_of(PLANAR, L, 3, "bytes", seed=6).reshape(3, 2, L, L, 4)
    want = site_twin(T, PLANAR, L, chains, cq)
    for fill in (0, 255):
        dirty = cq.copy()
        dirty[:, 1, -1, :] = fill
        dirty[:, 1, :, -1] = fill
        assert not np.array_equal(dirty, cq)
        assert all(np.array_equal(x, y) for x, y in zip(site_twin(T, PLANAR, L, chains, dirty), want))
    dirty = cq.copy()
    dirty[:, 0, 0, 0] ^= 0x55                                                   # a qubit: the costs move
    assert not np.array_equal(site_twin(T, PLANAR, L, chains, dirty)[0], want[0])


# ------------------------------------------------------------------------------------------------------ refusals
def test_the_cost_range_is_refused_by_name(T):
    zeros = lambda code, L, n=1: np.zeros((n, nq_of(code, L)), np.uint8)
    rc, msg, cost, _, _ = twin_rc(T, ROTATED, 21, zeros(ROTATED, 21), (0, 200, 1, 1))
    print(msg)
    assert rc == -4 and msg.startswith(PREFIX) and b"441 qubits" in msg and b"200" in msg and b"16 bits" in msg and np.all(cost == 77)
    assert 441 * 148 < 65536 <= 441 * 149
    assert twin_rc(T, ROTATED, 21, zeros(ROTATED, 21, 0), (0, 148, 1, 1))[0] == 0                        # (N == 0: the checks alone)
    assert twin_rc(T, ROTATED, 21, zeros(ROTATED, 21, 0), (149, 1, 1, 1))[0] == -4
    assert twin_rc(T, PLANAR, 12, zeros(PLANAR, 12, 0), (0, 247, 247, 247))[0] == 0 and 265 * 247 < 65536 <= 265 * 248
    assert twin_rc(T, PLANAR, 12, zeros(PLANAR, 12, 0), (0, 1, 248, 1))[0] == -4
    rc, msg, _, _, _ = twin_rc(T, ROTATED, 3, zeros(ROTATED, 3), (0, 1, 256, 1))
    assert rc == -1 and msg.startswith(PREFIX) and b"cost[2]=256" in msg
    assert twin_rc(T, ROTATED, 9, zeros(ROTATED, 9), (255, 255, 255, 255))[0] == 0                       # 81 qubits: every byte fits
    # a site row over the limit, named; the rows before it and the unused cells do not count
    code, L = PLANAR, 12
    nq = nq_of(code, L)
    cq = np.zeros((3, nq, 4), np.uint8)
    cq[:, :, 2] = 247                                                           # 265 * 247 = 65 455 in every row: within the limit
    cq.reshape(3, 2, L, L, 4)[1, 1, -1, :] = 255                                # unused cells of row 1: not priced (they would carry it past the limit)
    cq[2, :11, 1] = 255                                                         # eleven qubits of row 2, 8 more each: 65 543
    rc, msg, cost, _, _ = site_twin_rc(T, code, L, zeros(code, L, 3), cq)
    print(msg)
    assert rc == -4 and msg.startswith(SITE_PREFIX) and b"cq row 2" in msg and b"65543" in msg and b"16 bits" in msg and np.all(cost == 77)
    cq[1, :, 0] = 248
    rc, msg, _, _, _ = site_twin_rc(T, code, L, zeros(code, L, 3), cq)
    assert rc == -4 and b"cq row 1" in msg                                      # the first row that passes it
    assert site_twin_rc(T, code, L, zeros(code, L, 0), cq, rows=3)[0] == 0      # N == 0: no row is read


TILED_REFUSED = [(XZZX, 4, 0, 0, -1, [b"odd L"]), (TORIC, 4, 0, 0, -4, [b"even length"]), (TORIC, 9, 0, 0, -4, [b"37 generators wide", b"held generators", b"width 24"]),
                 (PLANAR, 13, 0, 0, -4, [b"26 generators wide", b"12 held generators leave width 25"]), (ROTATED, 23, 0, 0, -4, [b"26 generators wide"]),
                 (XZZX, 23, 0, 0, -4, [b"26 generators wide"]), (TORIC, 7, 16, 0, -4, [b"29 generators wide", b"width 16"]),
                 (ROTATED, 21, 13, 0, -4, [b"24 generators wide", b"12 held generators leave width"]), (XZZX, 3, 0, 3, -1, [b"tile_width=3"]),
                 (XZZX, 3, 0, 14, -1, [b"tile_width=14"]), (XZZX, 3, 25, 0, -1, [b"hbm_width=25"]), (XZZX, 3, 7, 8, -1, [b"hbm_width=7"]), (-1, 3, 0, 0, -1, []),
                 (TORIC, 65, 0, 0, -1, [])]


def test_tiled_plan_refusals_are_prefixed(T):
    for code, L, hw, tw, want, frags in TILED_REFUSED:
        nq = nq_of(code, L)
        rc0, _, plain = ST.info(T, code, L, hw, tw)
        rc, msg, cost, _, _ = twin_rc(T, code, L, np.zeros((1, nq), np.uint8), UNIT, hw, tw)
        print(code, L, hw, tw, msg)
        assert rc == rc0 == want and msg == PREFIX + b" " + plain and all(f in msg for f in frags) and np.all(cost == 77), (code, L, hw, tw, msg)
        rc, msg, cost, _, _ = site_twin_rc(T, code, L, np.zeros((1, nq), np.uint8), np.zeros((1, nq, 4), np.uint8), hw, tw)
        assert rc == want and msg == SITE_PREFIX + b" " + plain and np.all(cost == 77)
    chains, cq = np.zeros((3, 9), np.uint8), np.zeros((3, 9, 4), np.uint8)
    rc, msg, _, _, _ = site_twin_rc(T, ROTATED, 3, chains, None, rows=1)
    assert rc == -1 and msg.startswith(SITE_PREFIX) and b"NULL" in msg
    for rows in (0, 2, 4):
        rc, msg, cost, _, _ = site_twin_rc(T, ROTATED, 3, chains, cq, rows=rows)
        assert rc == -1 and msg.startswith(SITE_PREFIX) and b"cq_rows=%d" % rows in msg and b"one table (1) or one per syndrome (N=3)" in msg and np.all(cost == 77)
    for rows in (1, 3):
        assert site_twin_rc(T, ROTATED, 3, chains, cq, rows=rows)[0] == 0
    assert site_twin_rc(T, ROTATED, 3, chains[:0], cq, rows=7)[0] == 0          # N == 0: any rows
    # the entry points of before answer what they answered: the cut plans still refuse the tiled shapes by name, whatever the costs
    for code, L, costs, w, want, frags in M.REFUSED:
        rc, msg, _, _, _ = M.twin_rc(T, code, L, np.zeros((1, nq_of(code, L)), np.uint8), costs, w)
        assert rc == want and msg.startswith(b"qecmc_class_minplus:") and all(f in msg for f in frags), msg


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    assert lib.qecmc_abi_version() == 4
    big = np.zeros((1, 2 * 23 * 23), np.uint8)
    cq = np.zeros((1, 2 * 23 * 23, 4), np.uint8)
    cost, count, cls = np.zeros((1, 16), np.uint32), np.zeros((1, 16), np.uint64), np.zeros(1, np.int32)
    tail = (cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), L_.i32(cls))
    u32 = lambda c: np.array(c, np.uint32).ctypes.data_as(_u32p)
    uniform = lambda code, L, hw, tw, n=1, costs=UNIT: lib.qecmc_class_minplus_tiled(code, L, n, L_.u8(big), u32(costs), hw, tw, *tail)
    site = lambda code, L, hw, tw, n=1, rows=1, table=cq: lib.qecmc_class_minplus_tiled_site(code, L, n, L_.u8(big), None if table is None else L_.u8(table), rows, hw, tw, *tail)
    for call, prefix in ((uniform, PREFIX), (site, SITE_PREFIX)):
        for code, L, hw, tw, want, frags in TILED_REFUSED:
            assert call(code, L, hw, tw) == want
            err = lib.qecmc_last_error()
            assert err.startswith(prefix) and all(f in err for f in frags), err
    assert uniform(ROTATED, 21, 0, 0, costs=(0, 200, 1, 1)) == -4 and lib.qecmc_last_error().startswith(PREFIX) and b"441 qubits" in lib.qecmc_last_error()
    assert uniform(ROTATED, 3, 0, 0, costs=(0, 1, 1, 256)) == -1 and lib.qecmc_last_error().startswith(PREFIX + b" cost[3]=256")
    heavy = np.full((1, 2 * 23 * 23, 4), 255, np.uint8)
    assert site(ROTATED, 21, 0, 0, table=heavy) == -4 and lib.qecmc_last_error().startswith(SITE_PREFIX + b" cq row 0")
    assert site(ROTATED, 3, 0, 0, table=None) == -1 and lib.qecmc_last_error().startswith(SITE_PREFIX) and b"NULL" in lib.qecmc_last_error()
    assert site(ROTATED, 3, 0, 0, rows=2) == -1 and lib.qecmc_last_error().startswith(SITE_PREFIX + b" cq_rows=2")
    assert lib.qecmc_class_minplus_tiled(ROTATED, 3, 1, None, u32(UNIT), 0, 0, *tail) == -1 and b"NULL" in lib.qecmc_last_error()
    assert lib.qecmc_class_minplus_tiled(ROTATED, 3, 1, L_.u8(big), None, 0, 0, *tail) == -1
    assert lib.qecmc_class_minplus_tiled(ROTATED, 3, 1, L_.u8(big), u32(UNIT), 0, 0, None, tail[1], None) == -1
    assert lib.qecmc_class_minplus_tiled(ROTATED, 3, 1, L_.u8(big), u32(UNIT), 0, 0, tail[0], None, None) == -1
    # a valid call gets as far as the device lookup: no device, no CPU fallback; N == 0 succeeds where there is one
    have = L_.device_count() >= 1
    for call in (uniform, site):
        for n in (1, 0):
            assert call(ROTATED, 3, 0, 0, n=n) == (0 if have else -2)
        if not have:
            assert b"no CPU fallback" in lib.qecmc_last_error()
    if not have:
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.class_minplus_tiled("rotated", np.zeros((1, 3, 3), np.uint8))


# ------------------------------------------------------------------------------------------------------ the Python layer
class _TwinLibrary(MS._TwinLibrary):
    """the library with the (min, +) entry points answered by the host twins, the two tiled ones among them"""

    def qecmc_class_minplus_tiled(self, *args):
        return self._T.qt_class_minplus_tiled(*args, None, 0)

    def qecmc_class_minplus_tiled_site(self, *args):
        return self._T.qt_class_minplus_tiled_site(*args, None, 0)


def test_python_layer_shapes_dtypes_and_the_method_keyword(T, monkeypatch):
    import qecmc
    for name in ("class_minplus_tiled", "class_minplus_tiled_site"):
        assert getattr(qecmc, name) is getattr(ex, name) and name in qecmc.__all__
    real = L_.lib()
    monkeypatch.setattr(ex.L_, "lib", lambda: _TwinLibrary(real, T))
    for code, L, hw, tw in [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4), (PLANAR, 5, 0, 0)]:
        n, nq, ncls = 4, nq_of(code, L), 16 if code == TORIC else 4
        chains = chains_of(code, L, n, seed=7)
        cq = MS.tables_of(code, L, n, "bytes", seed=7)
        cost, count, cls = twin(T, code, L, chains, SPLIT, hw, tw)
        r = ex.class_minplus_tiled(NAME[code], chains, SPLIT, hbm_width=hw, tile_width=tw)
        assert set(r) == set(ex.class_minplus(NAME[code], chains)) | {"segments"}
        assert r["cost"].dtype == np.uint32 and r["count"].dtype == np.uint64 and r["cls"].dtype == np.int32 and r["saturated"].dtype == bool
        assert r["cost"].shape == r["count"].shape == r["saturated"].shape == (n, ncls) and r["cls"].shape == (n,)
        assert np.array_equal(r["cost"], cost) and np.array_equal(r["count"], count) and np.array_equal(r["cls"], cls) and not r["saturated"].any()
        inf = ST.info(T, code, L, hw, tw)[1]
        assert (r["width"], r["held"], r["segments"]) == (inf["width"], inf["held"], inf["segments"])
        flat = ex.class_minplus_tiled(code, chains.reshape(n, -1), SPLIT, size=L, hbm_width=hw, tile_width=tw)
        assert np.array_equal(flat["cost"], cost) and np.array_equal(flat["count"], count)
        scost, scount, scls = site_twin(T, code, L, chains, cq, hw, tw)
        m = ex.class_minplus_tiled_site(NAME[code], chains, cq.reshape((n,) + state_shape(code, L) + (4,)), hbm_width=hw, tile_width=tw)
        assert set(m) == set(r) and np.array_equal(m["cost"], scost) and np.array_equal(m["count"], scount) and np.array_equal(m["cls"], scls)
        one = ex.class_minplus_tiled_site(NAME[code], chains, cq[0], hbm_width=hw, tile_width=tw)
        assert np.array_equal(one["cost"], site_twin(T, code, L, chains, cq[:1], hw, tw)[0])
        # method="tiled": the same ranking and the same law as the cut route gives at these shapes -- and the widths reach the library
        kw = dict(method="tiled", hbm_width=hw, tile_width=tw)
        assert np.array_equal(ex.min_weight_classes(NAME[code], chains, SPLIT, **kw), ex._rank_classes(cost, count))
        assert np.array_equal(ex.min_weight_classes(NAME[code], chains, SPLIT, **kw), ex.min_weight_classes(NAME[code], chains, SPLIT))
        assert np.array_equal(ex.min_weight_classes_site(NAME[code], chains, cq, **kw), ex._rank_classes(scost, scount))
        assert np.array_equal(ex.shortest_class_law(NAME[code], chains, 0.05, **kw), ex.shortest_class_law(NAME[code], chains, 0.05))
        assert np.array_equal(ex.shortest_class_law(NAME[code], chains, 0.05, site_costs=cq, **kw), ex._law_from_minplus(scost, scount, scount == 0, (0.05 / 3.0) / 0.95))


def test_python_checks_its_arguments_and_the_library_refuses_by_name():
    chains = np.zeros((2, 3, 3), np.uint8)
    with pytest.raises(L_.QecmcError, match="qecmc_class_minplus_tiled: tile_width=3"):
        ex.min_weight_classes("rotated", chains, method="tiled", tile_width=3)
    with pytest.raises(L_.QecmcError, match="qecmc_class_minplus_tiled_site: hbm_width=25"):
        ex.min_weight_classes_site("rotated", chains, np.zeros((9, 4), np.uint8), method="tiled", hbm_width=25)
    with pytest.raises(ValueError, match="method='matching'"):
        ex.min_weight_classes("rotated", chains, method="matching")
    with pytest.raises(ValueError, match="lds_width belongs to method='cut'"):
        ex.shortest_class_law("rotated", chains, 0.1, method="tiled", lds_width=13)
    with pytest.raises(ValueError, match="hbm_width and tile_width belong to method='tiled'"):
        ex.min_weight_classes_site("rotated", chains, np.zeros((9, 4), np.uint8), tile_width=8)
    for bad in [(0, 1, 1), (0, 1.5, 1, 1), (0, -1, 1, 1)]:
        with pytest.raises(ValueError, match="integer costs"):
            ex.class_minplus_tiled("rotated", chains, bad)
    with pytest.raises(ValueError, match=r"site_costs\[row 0\]\[qubit 4\]\[Y\]=256.0"):
        table = np.zeros((3, 3, 4))
        table[1, 1, 2] = 256
        ex.class_minplus_tiled_site("rotated", chains, table)
    with pytest.raises(L_.QecmcError, match="qecmc_class_minplus_tiled: 441 qubits"):
        ex.class_minplus_tiled("rotated", np.zeros((1, 21, 21), np.uint8), (0, 200, 200, 200))


def test_harness_routes_min_weight_to_the_tiled_sweep_only_where_it_is_named(T, monkeypatch):
    real = L_.lib()
    calls = []

    class Spy(_TwinLibrary):
        def qecmc_class_minplus_tiled(self, *args):
            calls.append(("tiled", args[5], args[6]))
            return super().qecmc_class_minplus_tiled(*args)

        def qecmc_class_minplus(self, *args):
            calls.append(("cut", args[5]))
            return super().qecmc_class_minplus(*args)

        def qecmc_class_minplus_tiled_site(self, *args):
            calls.append(("tiled_site", args[6], args[7]))
            return super().qecmc_class_minplus_tiled_site(*args)

    monkeypatch.setattr(ex.L_, "lib", lambda: Spy(real, T))
    chains = chains_of(ROTATED, 7, 3, seed=8)
    params = dict(code="rotated", size=7, p_error=0.05, method="min_weight")
    want = harness._min_weight_distr(params, chains, 0)
    assert calls == [("cut", 0)]
    for other in ("auto", "cut", "sweep"):                                      # every other value is what it is today: the cut plans
        assert np.array_equal(harness._min_weight_distr(dict(params, exact_method=other, tile_width=5), chains, 0), want)
    assert calls == [("cut", 0)] * 4
    got = harness._min_weight_distr(dict(params, exact_method="tiled", hbm_width=12, tile_width=5), chains, 0)
    assert calls[-1] == ("tiled", 12, 5) and np.array_equal(got, want)
    cq = ex.erasure_site_costs((0, 1, 1, 1), np.random.default_rng(9).random((3, 7, 7)) < 0.2)
    got = harness._min_weight_distr(dict(params, exact_method="tiled", tile_width=6, site_costs=cq), chains, 0)
    assert calls[-1] == ("tiled_site", 0, 6) and np.array_equal(got, harness._min_weight_distr(dict(params, site_costs=cq), chains, 0))


def test_harness_refuses_the_traced_correction_under_the_tiled_route():
    params = dict(code="rotated", size=13, p_error=0.05, method="min_weight", exact_method="tiled", correction="shortest")
    with pytest.raises(ValueError, match="correction'\\]='shortest' is not built for params\\['exact_method'\\]='tiled'.*no traceback"):
        harness.generate(params, 2, corrections=True)
    with pytest.raises(ValueError, match="no traceback"):
        harness.decode_syndromes(params, np.zeros((1, 168), np.uint8), corrections=True)
    assert harness._correction_route(dict(params, exact_method="cut"), "min_weight") == "shortest"
    assert harness._correction_route(dict(params, correction=None), "min_weight") is None
    with pytest.raises(ValueError, match="min_weight is defined for depolarizing and alpha noise, not biased"):
        harness.erasure_experiment(dict(code="rotated", size=13, p_error=0.1, p_erase=0.1, noise="biased", eta=3.0, exact_method="tiled"), 2, method="min_weight")
