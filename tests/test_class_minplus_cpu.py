"""The shortest chain of every class and its multiplicity (the (min, +, count) sweep of csrc/class_minplus.hpp), without a GPU: the twin, compiled by
g++ into the host-table test library (qt_class_minplus, qt_minplus_combine), and the Python layer around it.

What is pinned: tests/util_minplus.py -- an elimination over the oracle's stencils that knows nothing of the planner, counts in Python integers --
against a brute force over the whole group at L = 3; the twin against that elimination under three cost vectors (unit costs, the alpha model's
(0, 3, 3, 1), and (1, 0, 2, 3): a cost of I, a free X, all four different); against the enumerator's twin histogram; at toric L = 5 against the
product of two sector brute forces; held generators change nothing; all-zero costs count the group, saturated past 2^48 - 1; the combine's algebra;
(cost, count) as a function of the syndrome alone; the low-p limit of the double twin; min_weight_classes; the refusals by name; the sanitizers.

Everything but the low-p limit is integer and compared exactly.  The low-p bound (relative 1e-5 at p = 1e-9) is the issue's: the two existing twins
differ from the nearest integer pair by 2.0e-7 at most over these inputs, the next-order term being A(d + 1) / A(d) * f with f = 3.3e-10; the bound
carries a x50 margin over that."""
import ctypes as C

import numpy as np
import pytest

import test_class_sweep_cpu as S
import test_class_sweep_cut_cpu as SC
import test_enumerate_cpu as E
from hostlib import run_selftest
from qecmc import _lib as L_
from qecmc import exact as ex
from test_corrections_cpu import classes, generators
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_minplus import brute_force_minplus, eliminate_minplus

NAME = S.NAME
UNIT, ALPHA3, MIXED = (0, 1, 1, 1), (0, 3, 3, 1), (1, 0, 2, 3)
COSTS = [UNIT, ALPHA3, MIXED]
K_SAT = (1 << 48) - 1
LOW_P = 1e-9
_u8p, _u32p, _i32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)


def load_twin():
    """the host-table test library with the min-plus entry points (tests/test_gpu_class_minplus.py compares the GPU with it)"""
    lib = SC.load_twin()
    lib.qt_class_minplus.restype = C.c_int
    lib.qt_class_minplus.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _u32p, C.c_int, _u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_minplus_combine.restype = C.c_uint64
    lib.qt_minplus_combine.argtypes = [C.c_uint64, C.c_uint64, _u64p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def twin_rc(T, code, L, chains, costs, lds_width=0):
    """(rc, message, cost uint32[N, ncls], count uint64[N, ncls], cls int32[N]) of the host twin on chains [N, ...]"""
    nq = int(np.prod(state_shape(code, L))) if 2 <= L <= 64 else 1
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    c = np.ascontiguousarray(costs, dtype=np.uint32)
    ncls = 16 if code == TORIC else 4
    cost, count, cls = np.full((len(flat), ncls), 77, np.uint32), np.full((len(flat), ncls), 77, np.uint64), np.full(len(flat), 9, np.int32)
    msg = C.create_string_buffer(640)
    rc = T.qt_class_minplus(code, L, len(flat), flat.ctypes.data_as(_u8p), c.ctypes.data_as(_u32p), lds_width, cost.ctypes.data_as(_u32p),
                            count.ctypes.data_as(_u64p), cls.ctypes.data_as(_i32p), msg, 640)
    return rc, msg.value, cost, count, cls


def twin(T, code, L, chains, costs, lds_width=0):
    rc, msg, cost, count, cls = twin_rc(T, code, L, chains, costs, lds_width)
    assert rc == 0, msg
    return cost, count, cls


def shift_of(code):
    """the generator table meets every chain 2^shift times: the torus has two dependent generators"""
    return 2 if code == TORIC else 0


def toric_order(L):
    """the torus' qubits row by row of the lattice in half steps, last row first (another order than the planner's, which starts at the first)"""
    key = lambda q: ((2 * (q % (L * L) // L) + 1, 2 * (q % L)) if q < L * L else (2 * (q % (L * L) // L), 2 * (q % L) + 1))
    return sorted(range(2 * L * L), key=key, reverse=True)


# ------------------------------------------------------------------------------------------------------ the utility is a brute force
@pytest.mark.parametrize("code", [TORIC, PLANAR, XZZX, ROTATED])
def test_the_elimination_of_util_minplus_is_a_brute_force_at_L3(code):
    gens = generators(code, 3)
    chains = random_errors(code, 3, 3, np.random.default_rng([41, code]))
    for chain in chains:
        for costs in COSTS:
            want = brute_force_minplus(gens, chain.ravel(), costs)
            assert eliminate_minplus(gens, chain.ravel(), costs, toric_order(3) if code == TORIC else None) == want
            assert want[1] % (1 << shift_of(code)) == 0 and want[1] > 0


# ------------------------------------------------------------------------------------------------------ the twin against the utility
@pytest.mark.parametrize("code,L", [(ROTATED, 7), (ROTATED, 9), (XZZX, 7), (PLANAR, 5)])
def test_twin_is_the_independent_elimination(T, code, L):
    """the input's own class and the classes reached through the oracle's logical operators"""
    chains = random_errors(code, L, 3, np.random.default_rng([42, code, L]))
    gens = generators(code, L)
    order = S.column_major(code, L) if code == PLANAR else None
    reps = [E.class_chains(code, m) for m in chains]                            # one chain per class, by the oracle's logical operators and class function
    for costs in COSTS:
        cost, count, cls = twin(T, code, L, chains, costs)
        assert np.array_equal(cls, classes(code, chains))
        for s in range(len(chains)):
            want = [eliminate_minplus(gens, r, costs, order) for r in reps[s]]
            print(NAME[code], L, costs, "syndrome", s, want)
            assert [(int(a), int(b)) for a, b in zip(cost[s], count[s])] == want


@pytest.mark.parametrize("seed", [0, 1])
def test_twin_is_the_independent_elimination_at_toric_L5(T, seed):
    """one chain each, its own class"""
    chain = random_errors(TORIC, 5, 2, np.random.default_rng([43, seed]))[1]    # (site error rate 0.15)
    gens = generators(TORIC, 5)
    costs = COSTS[seed]
    cost, count, cls = twin(T, TORIC, 5, chain[None], costs)
    c, n = eliminate_minplus(gens, chain.ravel(), costs, toric_order(5), max_axes=22)
    print("toric L=5", costs, "class", int(cls[0]), "cost", c, "count", n)
    assert n % 4 == 0 and (int(cost[0, cls[0]]), int(count[0, cls[0]])) == (c, n // 4)


# ------------------------------------------------------------------------------------------------------ the twin against the enumerator's histogram
@pytest.mark.parametrize("code,L", [(TORIC, 3), (ROTATED, 5), (PLANAR, 4)])
def test_twin_is_the_least_occupied_bin_of_the_enumerators_twin(T, code, L):
    """costs with c_X = c_Y are a function a n_xy + b n_z of the two counts the enumerator's histogram keeps: the least value over the occupied bins,
    and the sum of the bins that reach it"""
    if (code, L) == (PLANAR, 4):
        chains = random_errors(code, L, 2, np.random.default_rng([44, code, L]))[1:]
        hist = E.twin(T, code, L, chains)[0]
    else:
        chains, hist = S.enum_case(T, code, L)
    n = np.arange(hist.shape[-1], dtype=np.int64)
    for costs in [UNIT, ALPHA3, (0, 2, 2, 5), (0, 0, 0, 1)]:
        value = costs[1] * n[:, None] + costs[3] * n[None, :]
        cost, count, _ = twin(T, code, L, chains, costs)
        for s in range(len(chains)):
            for c in range(hist.shape[1]):
                occupied = hist[s, c] > 0
                least = value[occupied].min()
                assert (int(cost[s, c]), int(count[s, c])) == (int(least), int(hist[s, c][occupied & (value == least)].sum())), (s, c, costs)


# ------------------------------------------------------------------------------------------------------ toric L = 5 against two sector brute forces
_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.int64)
_sector = {}


def sector_minimum(gens, chain, bit):
    """(the least X-or-Y count (bit 0) or Z-or-Y count (bit 1) over all 2^25 subsets of the sector's generators, the number of subsets that reach it):
    brute force over the bit planes, as tests/test_class_sweep_cut_cpu.sector_sums walks them"""
    part = (lambda a: ((a == 1) | (a == 2))) if bit == 0 else (lambda a: (a >= 2))
    mine = [g for g in gens if (g == (1, 3)[bit]).any()]
    assert len(mine) == 25 and all(set(np.unique(g).tolist()) == {0, (1, 3)[bit]} for g in mine)
    rows = np.array([sum(1 << int(q) for q in np.flatnonzero(part(g))) for g in mine], dtype=np.uint64)
    start = np.uint64(sum(1 << int(q) for q in np.flatnonzero(part(chain))))
    if (bit, int(start)) in _sector:                                            # (classes that differ in the other sector alone share this one)
        return _sector[bit, int(start)]
    lo = np.zeros(1, np.uint64)
    for r in rows[:16]:
        lo = np.concatenate([lo, lo ^ r])
    hi = np.zeros(1, np.uint64)
    for r in rows[16:]:
        hi = np.concatenate([hi, hi ^ r])
    tally = np.zeros(51, np.int64)
    for h in hi:
        v = lo ^ (h ^ start)
        cnt = np.zeros(v.shape, np.int64)
        for k in range(0, 64, 16):
            cnt += _POP16[((v >> np.uint64(k)) & np.uint64(0xFFFF)).astype(np.int64)]
        tally += np.bincount(cnt, minlength=51)
    least = int(np.flatnonzero(tally)[0])
    _sector[bit, int(start)] = (least, int(tally[least]))
    return _sector[bit, int(start)]


def test_toric_L5_is_the_sum_and_the_product_of_its_two_sectors(T):
    """costs (0, 1, 2, 1): c_Y = c_X + c_Z, so the cost of a chain is its X-or-Y count plus its Z-or-Y count, the torus' vertex generators move the
    first alone and its plaquette generators the second: cost is the sum of the two sector minima and count the product of their multiplicities --
    every element is met twice in either sector.  Three classes of one syndrome, widths 13 (8 held) and 14 (7 held)."""
    chain = random_errors(TORIC, 5, 2, np.random.default_rng(545))[1]
    gens = generators(TORIC, 5)
    cost, count, cls = twin(T, TORIC, 5, chain[None], (0, 1, 2, 1), 13)
    reps = E.class_chains(TORIC, chain)
    for c in (int(cls[0]), (int(cls[0]) + 5) % 16, (int(cls[0]) + 10) % 16):
        (cx, nx), (cz, nz) = sector_minimum(gens, reps[c], 0), sector_minimum(gens, reps[c], 1)
        print("class %d: twin (%d, %d); sectors (%d, %d) and (%d, %d)" % (c, cost[0, c], count[0, c], cx, nx, cz, nz))
        assert nx % 2 == 0 and nz % 2 == 0
        assert (int(cost[0, c]), int(count[0, c])) == (cx + cz, (nx // 2) * (nz // 2))
    cost14, count14, _ = twin(T, TORIC, 5, chain[None], (0, 1, 2, 1), 14)
    assert np.array_equal(cost14, cost) and np.array_equal(count14, count)


# ------------------------------------------------------------------------------------------------------ held generators, the group, saturation
def test_held_generators_change_nothing(T):
    chains = random_errors(TORIC, 3, 6, np.random.default_rng([45]))
    for costs in COSTS:
        want = twin(T, TORIC, 3, chains, costs, 0)
        assert SC.info(T, TORIC, 3, 0)[1]["held"] == 0
        for w in (6, 9, 12):
            assert SC.info(T, TORIC, 3, w)[1]["held"] >= 1                      # (the torus at L = 3 is 13 wide)
            got = twin(T, TORIC, 3, chains, costs, w)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (costs, w)


def test_all_zero_costs_count_the_group_and_saturate_past_48_bits(T):
    cost, count, _ = twin(T, ROTATED, 5, random_errors(ROTATED, 5, 2, np.random.default_rng(46)), (0, 0, 0, 0))
    assert np.all(cost == 0) and np.all(count == 1 << 24)
    cost, count, _ = twin(T, TORIC, 3, random_errors(TORIC, 3, 2, np.random.default_rng(47)), (0, 0, 0, 0))
    assert np.all(cost == 0) and np.all(count == 1 << 16)                       # 2^18 subsets, shifted by 2
    chains = random_errors(ROTATED, 7, 2, np.random.default_rng(48))
    cost, count, cls = twin(T, ROTATED, 7, chains, (0, 0, 0, 0))                # 2^48 > kSat
    assert np.all(cost == 0) and np.all(count == 0)
    with pytest.raises(OverflowError, match="row 0"):
        ex._law_from_minplus(cost, count, count == 0, 0.1)
    cost, count, _ = twin(T, ROTATED, 7, chains, (5, 5, 5, 5))                  # (a constant cost: the same count, at cost 5 * 49)
    assert np.all(cost == 5 * 49) and np.all(count == 0)
    cost, count, _ = twin(T, ROTATED, 7, chains, UNIT)                          # ... and real costs at the same shape are far from it
    assert np.all(count > 0) and count.max() < 1 << 30


def test_combine_tie_rule_saturation_and_associativity(T):
    out3 = np.zeros(3, np.uint64)
    comb = lambda a, b: int(T.qt_minplus_combine(a, b, None))
    pack = lambda cost, count: (cost << 48) | count
    assert comb(pack(3, 5), pack(4, 9)) == pack(3, 5) == comb(pack(4, 9), pack(3, 5))
    assert comb(pack(3, 5), pack(3, 9)) == pack(3, 14)
    T.qt_minplus_combine(0, 0, out3.ctypes.data_as(_u64p))
    assert out3.tolist() == [K_SAT, 48, 255]
    assert comb(pack(7, K_SAT), pack(7, 1)) == pack(7, K_SAT) == comb(pack(7, K_SAT - 1), pack(7, 1)) == comb(pack(7, K_SAT), pack(7, K_SAT))
    assert comb(pack(7, K_SAT - 2), pack(7, 1)) == pack(7, K_SAT - 1)
    assert comb(pack(7, K_SAT), pack(6, 1)) == pack(6, 1)                       # (a cheaper entry replaces a saturated one)
    assert comb(pack(0xFFFF, 1), pack(0xFFFF, 2)) == pack(0xFFFF, 3)
    rng = np.random.default_rng(49)
    for _ in range(3000):
        e = []
        for how in rng.integers(4, size=3):
            n = [1 + int(rng.integers(7)), K_SAT - int(rng.integers(5)), (K_SAT >> 1) + int(rng.integers(3)), 1 + int(rng.integers(1 << 47))][how]
            e.append(pack(int(rng.integers(3)), n))
        assert comb(comb(e[0], e[1]), e[2]) == comb(e[0], comb(e[1], e[2])) and comb(e[0], e[1]) == comb(e[1], e[0])
        # ... against the definition in Python integers
        least = min(x >> 48 for x in e)
        assert comb(comb(e[0], e[1]), e[2]) == pack(least, min(sum(x & K_SAT for x in e if x >> 48 == least), K_SAT))


@pytest.mark.parametrize("code,L,lds_width", [(TORIC, 3, 8), (XZZX, 5, 0), (PLANAR, 4, 6), (ROTATED, 7, 0)])
def test_cost_and_count_are_functions_of_the_syndrome(T, code, L, lds_width):
    """three representatives of one syndrome -- the chain, the chain times seven generators, and that a logical operator away -- agree entry for entry:
    the columns are indexed by the class itself"""
    chains = random_errors(code, L, 3, np.random.default_rng([50, code, L]))
    gens, rng = generators(code, L), np.random.default_rng([51, code, L])
    moved = chains.copy()
    for s in range(len(moved)):
        for g in rng.integers(len(gens), size=7):
            moved[s] ^= gens[g].reshape(moved[s].shape)
    for costs in COSTS:
        cost, count, cls = twin(T, code, L, chains, costs, lds_width)
        ncls = cost.shape[1]
        other = np.stack([E.class_chains(code, m)[(c + 1) % ncls].reshape(m.shape) for m, c in zip(moved, cls)])
        c1, n1, k1 = twin(T, code, L, moved, costs, lds_width)
        c2, n2, k2 = twin(T, code, L, other, costs, lds_width)
        assert np.array_equal(c1, cost) and np.array_equal(n1, count) and np.array_equal(k1, cls)
        assert np.array_equal(c2, cost) and np.array_equal(n2, count) and np.array_equal(k2, (cls + 1) % ncls)


# ------------------------------------------------------------------------------------------------------ the low-p limit of the double twin
_low_p = {}


def low_p_case(T, code, L):
    """60 random chains of one shape: the min-plus twin at unit costs and the double twin's Z at p = 1e-9, computed once"""
    if (code, L) not in _low_p:
        chains = random_errors(code, L, 60, np.random.default_rng([52, code, L]))
        cost, count, cls = twin(T, code, L, chains, UNIT)
        z, zcls = S.twin(T, code, L, chains, ex.depolarizing_w4(LOW_P))
        assert np.array_equal(cls, zcls)
        _low_p[code, L] = (cost, count, z)
    return _low_p[code, L]


LOW_P_SHAPES = [(ROTATED, 7), (ROTATED, 9), (XZZX, 9), (PLANAR, 6)]


@pytest.mark.parametrize("code,L", LOW_P_SHAPES)
def test_low_p_limit_of_the_class_weights(T, code, L):
    cost, count, z = low_p_case(T, code, L)
    f = (LOW_P / 3.0) / (1.0 - LOW_P)
    want = count.astype(np.float64) * f ** cost.astype(np.float64)
    diff = np.abs(want - z) / z
    print(NAME[code], L, "largest relative difference %.3g, smallest Z %.3g, largest count %d" % (diff.max(), z.min(), count.max()))
    assert z.min() > 0 and diff.max() <= 1e-5


@pytest.mark.parametrize("code,L", LOW_P_SHAPES)
def test_min_weight_classes_is_the_argmax_of_the_law_at_low_p(T, code, L):
    """rows whose two best classes tie in both cost and count are left out (the law at p = 1e-9 does not tell them apart either); their share stays
    <= 25 %"""
    cost, count, z = low_p_case(T, code, L)
    got = ex._rank_classes(cost, count)
    order = np.lexsort((-count.astype(np.int64), cost.astype(np.int64)), axis=1)
    rows = np.arange(len(cost))
    best, second = order[:, 0], order[:, 1]
    tied = (cost[rows, best] == cost[rows, second]) & (count[rows, best] == count[rows, second])
    print(NAME[code], L, "rows left out: %d of %d" % (tied.sum(), len(tied)))
    assert tied.mean() <= 0.25
    assert np.array_equal(got[~tied], np.argmax(z, axis=1)[~tied])
    assert np.array_equal(got[tied], np.minimum(best, second)[tied])            # (a full tie goes to the lower class index)
    law = ex._law_from_minplus(cost, count, count == 0, (LOW_P / 3.0) / (1.0 - LOW_P))
    assert np.abs(law - z / z.sum(axis=1, keepdims=True)).max() <= 1e-5 and np.allclose(law.sum(axis=1), 1.0, atol=1e-12)


def test_rank_classes_breaks_ties_by_count_then_index():
    cost = np.array([[3, 2, 2, 2], [1, 1, 1, 1], [4, 4, 0, 9]], np.uint32)
    count = np.array([[5, 1, 7, 7], [2, 3, 3, 1], [1, 1, 1, 1]], np.uint64)
    assert ex._rank_classes(cost, count).tolist() == [2, 1, 2] and ex._rank_classes(cost, count).dtype == np.int32
    law = ex._law_from_minplus(np.array([[700, 702, 701, 9999]], np.uint32), np.array([[2, 300, 5, 1]], np.uint64), np.zeros((1, 4), bool), 0.1)
    assert np.allclose(law, np.array([[2.0, 3.0, 0.5, 0.0]]) / 5.5)             # relative to the row's least cost: nothing underflows


# ------------------------------------------------------------------------------------------------------ refusals
REFUSED = [(ROTATED, 3, (0, 1, 256, 1), 0, -1, [b"cost[2]=256"]), (TORIC, 4, UNIT, 0, -4, [b"even length"]), (TORIC, 7, UNIT, 0, -4, [b"held generators"]),
           (ROTATED, 13, UNIT, 0, -4, [b"held generators", b"16 generators wide"]), (ROTATED, 3, UNIT, 15, -1, [b"lds_width"]),
           (ROTATED, 3, UNIT, 1, -1, [b"lds_width"]), (PLANAR, 8, UNIT, 14, -4, [b"held generators"]), (XZZX, 4, UNIT, 0, -1, [b"odd L"])]


def test_refusals_by_name(T):
    for code, L, costs, w, want, frags in REFUSED:
        rc, msg, _, _, _ = twin_rc(T, code, L, np.zeros((1, int(np.prod(state_shape(code, L)))), np.uint8), costs, w)
        print(NAME[code], L, costs, w, msg)
        assert rc == want and msg.startswith(b"qecmc_class_minplus:") and all(f in msg for f in frags), (code, L, w, msg)
    assert twin_rc(T, ROTATED, 3, np.zeros((1, 9), np.uint8), (255, 255, 255, 255))[0] == 0
    assert T.qt_class_minplus(ROTATED, 3, 1, None, None, 0, None, None, None, None, 0) == -1


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    assert lib.qecmc_abi_version() == 4
    big = np.zeros((1, 2 * 13 * 13), np.uint8)
    cost, count, cls = np.zeros((1, 16), np.uint32), np.zeros((1, 16), np.uint64), np.zeros(1, np.int32)
    u32 = lambda c: np.array(c, np.uint32).ctypes.data_as(_u32p)
    call = lambda code, L, costs, w, n=1: lib.qecmc_class_minplus(code, L, n, L_.u8(big), u32(costs), w, cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), L_.i32(cls))
    for code, L, costs, w, want, frags in REFUSED:
        assert call(code, L, costs, w) == want
        err = lib.qecmc_last_error()
        assert err.startswith(b"qecmc_class_minplus:") and all(f in err for f in frags), err
    assert lib.qecmc_class_minplus(ROTATED, 3, 1, None, u32(UNIT), 0, cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert lib.qecmc_class_minplus(ROTATED, 3, 1, L_.u8(big), None, 0, cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), None) == -1
    assert lib.qecmc_class_minplus(ROTATED, 3, 1, L_.u8(big), u32(UNIT), 0, None, count.ctypes.data_as(_u64p), None) == -1
    assert lib.qecmc_class_minplus(ROTATED, 3, 1, L_.u8(big), u32(UNIT), 0, cost.ctypes.data_as(_u32p), None, None) == -1
    # a valid call gets as far as the device lookup: no device, no CPU fallback
    have = L_.device_count() >= 1
    for n in (1, 0):
        assert call(ROTATED, 3, UNIT, 0, n) == (0 if have else -2)
    if not have:
        assert b"no CPU fallback" in lib.qecmc_last_error()
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.class_minplus("rotated", np.zeros((1, 3, 3), np.uint8))


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_python_checks_its_arguments_before_the_library():
    import qecmc
    assert qecmc.class_minplus is ex.class_minplus and qecmc.min_weight_classes is ex.min_weight_classes and qecmc.shortest_class_law is ex.shortest_class_law
    chains = np.zeros((2, 3, 3), np.uint8)
    for bad in [(0, 1, 1), (0, 1, 1, 1, 1), (0, 1.5, 1, 1), (0, -1, 1, 1)]:
        with pytest.raises(ValueError, match="integer costs"):
            ex.class_minplus("rotated", chains, bad)
    with pytest.raises(ValueError, match="not \\[N, \\.\\.\\.\\] configurations"):
        ex.class_minplus("toric", np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(L_.QecmcError, match="cost\\[3\\]=256"):
        ex.class_minplus("rotated", chains, (0, 1, 1, 256))
    with pytest.raises(L_.QecmcError, match="qecmc_class_minplus: .*held generators"):
        ex.min_weight_classes("toric", np.zeros((1, 2, 7, 7), np.uint8))
    with pytest.raises(L_.QecmcError, match="lds_width"):
        ex.class_minplus("rotated", chains, lds_width=15)
    with pytest.raises(ValueError, match="integer-valued alpha"):
        ex.shortest_class_law("rotated", chains, 0.3, alpha=2.5)
    with pytest.raises(ValueError, match="integer-valued alpha"):
        ex.shortest_class_law("rotated", chains, 0.3, alpha=256)


def test_harness_refusals():
    from qecmc import harness
    with pytest.raises(ValueError, match="min_weight is defined for depolarizing and alpha noise, not biased"):
        harness.generate(dict(code="rotated", size=5, p_error=0.1, noise="biased", eta=3.0, method="min_weight"), 4)
    with pytest.raises(ValueError, match="min_weight is defined for depolarizing and alpha noise, not biased"):
        harness._min_weight_distr(dict(code="rotated", size=5, p_error=0.1, noise="biased", eta=3.0), np.zeros((1, 5, 5), np.uint8), 0)
    with pytest.raises(ValueError, match="toric code is defined for depolarizing noise"):
        harness._min_weight_distr(dict(code="toric", size=3, p_error=0.1, noise="alpha", alpha=2), np.zeros((1, 2, 3, 3), np.uint8), 0)
    with pytest.raises(ValueError, match="device 0"):
        harness._min_weight_distr(dict(code="rotated", size=5, p_error=0.1), np.zeros((1, 5, 5), np.uint8), 1)
    with pytest.raises(ValueError, match="integer-valued alpha"):
        harness._min_weight_distr(dict(code="rotated", size=5, p_error=0.3, noise="alpha", alpha=1.5), np.zeros((1, 5, 5), np.uint8), 0)
    with pytest.raises(ValueError, match="PTEQ, exact and min_weight"):
        harness.generate(dict(code="rotated", size=5, p_error=0.1, method="STDC"), 4, start="syndrome")


# ------------------------------------------------------------------------------------------------------ the sanitizers
def test_minplus_under_sanitizers():
    """a stand-alone program (its own main) built from class_minplus.hpp with -fsanitize=address,undefined: every plan, accepted or refused, against the
    cut plan; the twin over poisoned scratch, threaded and not, held and not, against a brute force; saturation; run as a child process"""
    run_selftest("minplus_asan", "class_minplus_selftest_asan")
