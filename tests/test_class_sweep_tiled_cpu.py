"""The frontier sweep on a state vector tiled over HBM, without a GPU: the planner, the segment table and the twin of csrc/class_sweep_tiled.hpp,
compiled by g++ into the host-table test library (qt_class_sweep_tiled_info, _ops, _segments, _held, qt_class_sweep_tiled), and the Python layer.

What is pinned: the invariants of the tiled plan against the oracle's stencils (held and swept generators partition the table; every swept generator
lives in one slot from before its first qubit to after its last; every qubit is closed once naming its swept generators; peak = width <= hbm_width)
and of its segment table (the segments partition the ops in order; every INTRO / FORGET slot of a segment lies in its tile bits T, |T| = tile_width;
the slots outside T do not change within a segment; the live-tile count is what the masks imply); the twin against the shipped twins BIT FOR BIT
where the stream is theirs, and to 1e-12 where forced holds split the sum another way; all-ones weights give exactly 2^rank at rotated L = 13, 17
and planar L = 8; a NumPy variable elimination over the oracle's stencils in reversed qubit order at rotated L = 13; the refusals by name, the old
entry points' among them; resolve_method as it was.

Tolerance 1e-12 relative per class weight, as tests/test_class_sweep_cut_cpu.py: all terms are positive and either side errs by about
(nq + G) 2^-53 -- 7e-14 at rotated L = 13."""
import ctypes as C

import numpy as np
import pytest

import test_class_sweep_cpu as S
import test_class_sweep_cut_cpu as SC
from hostlib import run_selftest
from qecmc import _lib as L_
from qecmc import exact as ex
from test_corrections_cpu import classes, generators
from test_enumerate_cpu import class_chains
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape

NAME = S.NAME
INTRO, CLOSE, FORGET = 0, 1, 2
MAX_HELD = 12
_u8p, _u32p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double)
# every accepted (code, L, hbm_width, tile_width) the tests of this file and of tests/test_gpu_class_sweep_tiled.py use
ACCEPTED = [(XZZX, 5, 0, 4), (TORIC, 3, 0, 6), (TORIC, 3, 0, 13), (ROTATED, 7, 0, 5), (TORIC, 5, 13, 0), (TORIC, 5, 16, 8), (ROTATED, 9, 0, 8), (ROTATED, 9, 0, 13),
            (ROTATED, 13, 0, 0), (ROTATED, 13, 0, 8), (ROTATED, 17, 0, 0), (PLANAR, 8, 0, 0), (PLANAR, 12, 0, 0), (ROTATED, 21, 0, 0), (XZZX, 21, 0, 0),
            (TORIC, 7, 0, 0), (TORIC, 7, 22, 0), (TORIC, 7, 20, 0)]
INFO_KEYS = ("full_width", "width", "held", "ncls", "nq", "n_ops", "rank", "n_gen", "segments", "state_bits", "hbm_width", "tile_width", "max_held",
             "max_width", "pass_units", "threads")


def load_twin():
    """the host-table test library with the tiled sweep's entry points (tests/test_gpu_class_sweep_tiled.py compares the GPU with it)"""
    lib = SC.load_twin()
    lib.qt_class_sweep_tiled_info.restype = C.c_int
    lib.qt_class_sweep_tiled_info.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _i32p, C.c_char_p, C.c_int]
    for name in ("qt_class_sweep_tiled_ops", "qt_class_sweep_tiled_segments"):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _u32p, C.c_int]
    lib.qt_class_sweep_tiled_held.restype = C.c_int
    lib.qt_class_sweep_tiled_held.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _u32p, C.c_int]
    lib.qt_class_sweep_tiled.restype = C.c_int
    lib.qt_class_sweep_tiled.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _f64p, C.c_int, C.c_int, _f64p, _i32p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def info(T, code, L, hbm_width=0, tile_width=0):
    """(rc, dict of INFO_KEYS, message)"""
    v, msg = np.zeros(16, np.int32), C.create_string_buffer(512)
    rc = T.qt_class_sweep_tiled_info(code, L, hbm_width, tile_width, v.ctypes.data_as(_i32p), msg, 512)
    return rc, dict(zip(INFO_KEYS, v.tolist())), msg.value


def twin(T, code, L, chains, w, hbm_width=0, tile_width=0):
    """the host twin on chains [N, ...] -> (Z float64[N, ncls], cls int32[N])"""
    nq = int(np.prod(state_shape(code, L)))
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    w = np.ascontiguousarray(w, dtype=np.float64)
    z, cls = np.full((len(flat), 16 if code == TORIC else 4), -1.0), np.full(len(flat), 9, np.int32)
    rc = T.qt_class_sweep_tiled(code, L, len(flat), flat.ctypes.data_as(_u8p), w.ctypes.data_as(_f64p), hbm_width, tile_width, z.ctypes.data_as(_f64p),
                                cls.ctypes.data_as(_i32p))
    assert rc == 0, rc
    return z, cls


def ops_of(T, code, L, hbm_width=0, tile_width=0):
    """the wide op stream as test_class_sweep_cpu.ops_of gives the narrow one: (kind, slot, top, mask, [(slot, Pauli)], qubit)"""
    _, inf, _ = info(T, code, L, hbm_width, tile_width)
    buf = np.zeros(4 * inf["n_ops"], np.uint32)
    assert T.qt_class_sweep_tiled_ops(code, L, hbm_width, tile_width, buf.ctypes.data_as(_u32p), buf.size) == buf.size
    out = []
    for w0, mask, pairs, qubit in buf.reshape(-1, 4).tolist():
        pr = [((pairs >> 8 * j) & 31, (pairs >> (8 * j + 5)) & 7) for j in range((w0 >> 9) & 7)]
        out.append((w0 & 15, (w0 >> 4) & 31, (w0 >> 12) & 31, mask, [(s, xz ^ (xz >> 1)) for s, xz in pr], qubit))
    return out


def segments_of(T, code, L, hbm_width=0, tile_width=0):
    """the segment table as dicts(op_first, op_count, tile, live, live_in, live_out, n_tiles)"""
    _, inf, _ = info(T, code, L, hbm_width, tile_width)
    buf = np.zeros(8 * inf["segments"], np.uint32)
    assert T.qt_class_sweep_tiled_segments(code, L, hbm_width, tile_width, buf.ctypes.data_as(_u32p), buf.size) == buf.size
    return [dict(zip(("op_first", "op_count", "tile", "live", "live_in", "live_out", "n_tiles"), row[:7])) for row in buf.reshape(-1, 8).tolist()]


def held_of(T, code, L, hbm_width=0, tile_width=0):
    """(table indices int32[n_held], the held generators as byte chains uint8[n_held, nq])"""
    _, inf, _ = info(T, code, L, hbm_width, tile_width)
    W = (inf["nq"] + 15) // 16
    index, words = np.full(MAX_HELD, -1, np.int32), np.zeros(MAX_HELD * W, np.uint32)
    n = T.qt_class_sweep_tiled_held(code, L, hbm_width, tile_width, index.ctypes.data_as(_i32p), words.ctypes.data_as(_u32p), words.size)
    assert n == inf["held"]
    words = words[:n * W].reshape(n, W)
    q = np.arange(inf["nq"])
    return index[:n], ((words[:, q >> 4] >> ((q & 15) * 2).astype(np.uint32)) & 3).astype(np.uint8)


def bits(v):
    return bin(v).count("1")


# ------------------------------------------------------------------------------------------------------ the plan and its segments
@pytest.mark.parametrize("code,L,hbm_width,tile_width", ACCEPTED)
def test_tiled_plan_and_segment_invariants(T, code, L, hbm_width, tile_width):
    rc, inf, msg = info(T, code, L, hbm_width, tile_width)
    assert rc == 0, msg
    gens = generators(code, L)
    print("%s L=%d hbm_width %d tile_width %d: full width %d, held %d, width %d, %d ops, %d segments" % (
        NAME[code], L, hbm_width, tile_width, inf["full_width"], inf["held"], inf["width"], inf["n_ops"], inf["segments"]))
    assert inf["max_held"] == MAX_HELD and inf["max_width"] == 24 and inf["held"] <= MAX_HELD
    assert inf["hbm_width"] == (hbm_width or 24) and inf["tile_width"] == (tile_width or 11) and 4 <= inf["tile_width"] <= 13
    assert inf["width"] <= inf["hbm_width"] <= 24 and inf["state_bits"] == max(inf["width"], inf["tile_width"])
    assert inf["full_width"] == S.info(T, code, L)[1]["width"]                  # the uncut planner's, also where that one refuses the width
    assert inf["held"] >= inf["full_width"] - inf["hbm_width"] and (inf["held"] == 0) == (inf["full_width"] <= inf["hbm_width"])
    assert inf["n_gen"] == len(gens) and inf["rank"] == (len(gens) - 2 if code == TORIC else len(gens))
    assert 1 <= inf["pass_units"] <= 65535 and (inf["pass_units"] * 8 << inf["state_bits"]) <= 1 << 30 and inf["threads"] in (64, 256, 1024)
    index, held = held_of(T, code, L, hbm_width, tile_width)
    assert len(set(index.tolist())) == len(index) and np.all(np.diff(index) > 0) and np.all((index >= 0) & (index < len(gens)))
    assert np.array_equal(held, gens[index])                                    # held_words[j] is generator index[j]'s Paulis
    swept = [g for g in range(len(gens)) if g not in set(index.tolist())]       # held and swept: disjoint, and together the table
    sw = gens[swept]
    at = [[int(g[q]) for g in sw if g[q]] for q in range(gens.shape[1])]
    ops = ops_of(T, code, L, hbm_width, tile_width)
    live, lifetimes, closed, peak, occupied = {}, [], [], 0, []
    for kind, slot, top, mask, pairs, qubit in ops:
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
            assert sorted(p for _, p in pairs) == sorted(at[qubit])             # exactly its generators that are not held
        else:
            assert kind == FORGET and slot in live and top > slot
            lifetimes.append(frozenset(live.pop(slot)))
            assert mask == sum(1 << s for s in live) and mask >> top == 0
        occupied.append((before, sum(1 << s for s in live)))
    assert not live and peak == inf["width"]
    assert sorted(closed) == [q for q in range(gens.shape[1]) if gens[:, q].any()]      # every qubit once, also one only held generators touch
    supports = [frozenset((q, int(g[q])) for q in np.flatnonzero(g)) for g in sw]
    assert sorted(map(sorted, lifetimes)) == sorted(map(sorted, supports))      # one lifetime per swept generator, covering exactly its qubits
    # ---- the segments
    segs = segments_of(T, code, L, hbm_width, tile_width)
    low = (1 << min(4, inf["tile_width"] - 1)) - 1
    nxt = 0
    for sg in segs:
        assert sg["op_first"] == nxt and sg["op_count"] >= 1                    # they partition the ops in order
        mine = range(nxt, nxt + sg["op_count"])
        nxt += sg["op_count"]
        tile = sg["tile"]
        assert bits(tile) == inf["tile_width"] and tile >> inf["state_bits"] == 0 and tile & low == low
        assert all((tile >> ops[o][1]) & 1 for o in mine if ops[o][0] != CLOSE)  # every INTRO / FORGET slot lies in T
        assert sg["live_in"] == occupied[mine[0]][0] and sg["live_out"] == occupied[mine[-1]][1]
        union = 0
        for o in mine:
            union |= occupied[o][0] | occupied[o][1]
            assert occupied[o][0] & ~tile == occupied[o][1] & ~tile == sg["live_in"] & ~tile         # the fixed slots do not change: a tile is live throughout
        assert sg["live"] == union and sg["n_tiles"] == 1 << bits(union & ~tile)
    assert nxt == len(ops) and segs[0]["live_in"] == 0 and segs[-1]["live_out"] == 0 and segs[0]["n_tiles"] == segs[-1]["n_tiles"] == 1


def test_segments_are_longest_runs(T):
    """greedy: the first INTRO / FORGET slot after a segment is outside the slots that segment used next to the low bits -- and they fill the tile"""
    for code, L, hw, tw in [(ROTATED, 13, 0, 0), (ROTATED, 13, 0, 8), (XZZX, 5, 0, 4), (TORIC, 5, 16, 8)]:
        inf, ops, segs = info(T, code, L, hw, tw)[1], ops_of(T, code, L, hw, tw), segments_of(T, code, L, hw, tw)
        low = (1 << min(4, inf["tile_width"] - 1)) - 1
        for sg in segs[:-1]:
            used = low
            for o in range(sg["op_first"], sg["op_first"] + sg["op_count"]):
                if ops[o][0] != CLOSE:
                    used |= 1 << ops[o][1]
            nxt = ops[sg["op_first"] + sg["op_count"]]
            assert nxt[0] != CLOSE and not (used >> nxt[1]) & 1 and bits(used) == inf["tile_width"], (code, L, sg)


def test_what_the_planner_reports(T):
    """the planner's own numbers (DESIGN.md 4.1m has the table)"""
    got = {(NAME[c], L, hw, tw): tuple(info(T, c, L, hw, tw)[1][k] for k in ("full_width", "held", "width", "n_ops", "segments")) for c, L, hw, tw in ACCEPTED}
    print(got)
    assert got["rotated", 13, 0, 0][:4] == (16, 0, 16, 505) and got["rotated", 17, 0, 0][:4] == (20, 0, 20, 865)
    assert got["rotated", 21, 0, 0][:4] == (24, 0, 24, 1321) and got["xzzx", 21, 0, 0][:3] == (24, 0, 24)
    assert got["planar", 8, 0, 0][:4] == (16, 0, 16, 337) and got["planar", 12, 0, 0][:4] == (24, 0, 24, 793)
    assert got["toric", 7, 0, 0][:3] == (29, 5, 24) and got["toric", 7, 22, 0][:3] == (29, 7, 22) and got["toric", 7, 20, 0][:3] == (29, 9, 20)
    assert got["toric", 5, 16, 8][:3] == (21, 5, 16) and got["toric", 5, 13, 0][:3] == (21, 8, 13)
    assert got["toric", 3, 0, 13][4] == 1 and got["toric", 3, 0, 6][4] > 1      # a stream that fits one tile is one segment
    assert got["rotated", 13, 0, 8][4] > got["rotated", 13, 0, 0][4]


def test_sweep_tiled_info_of_the_python_layer():
    want = {("rotated", 13): (16, 0, 16), ("rotated", 21): (24, 0, 24), ("toric", 7): (29, 5, 24)}
    for (code, L), v in want.items():
        inf = ex.sweep_tiled_info(code, L)
        assert (inf["full_width"], inf["held"], inf["width"]) == v and inf["segments"] >= 1 and inf["ncls"] == (16 if code == "toric" else 4)
    import qecmc
    assert qecmc.sweep_tiled_info is ex.sweep_tiled_info and qecmc.class_sweep_tiled is ex.class_sweep_tiled


# ------------------------------------------------------------------------------------------------------ the twin against the shipped twins
@pytest.mark.parametrize("code,L,tile_width", [(TORIC, 3, 6), (TORIC, 3, 13), (XZZX, 5, 4), (ROTATED, 7, 5)])
def test_with_nothing_held_the_tiled_twin_is_the_sweep_twin_bit_for_bit(T, code, L, tile_width):
    assert info(T, code, L, 0, tile_width)[1]["held"] == 0
    chains = random_errors(code, L, 3, np.random.default_rng([41, code, L]))
    z, cls = twin(T, code, L, chains, S.SKEW, 0, tile_width)
    want, wcls = S.twin(T, code, L, chains, S.SKEW)
    assert np.array_equal(z.view(np.uint64), want.view(np.uint64)) and np.array_equal(cls, wcls) and np.array_equal(cls, classes(code, chains))
    narrow, wide = S.ops_of(T, code, L), ops_of(T, code, L, 0, tile_width)      # the same stream in the other encoding
    assert narrow == wide


def test_toric_L5_with_the_cut_plans_holds_is_the_cut_twin_bit_for_bit(T):
    chains = random_errors(TORIC, 5, 1, np.random.default_rng([42, 5]))
    z, cls = twin(T, TORIC, 5, chains, S.SKEW, 13, 0)
    want, wcls = SC.twin(T, TORIC, 5, chains, S.SKEW, 13)
    assert np.array_equal(z.view(np.uint64), want.view(np.uint64)) and np.array_equal(cls, wcls)
    assert np.array_equal(held_of(T, TORIC, 5, 13, 0)[0], SC.held_of(T, TORIC, 5, 13)[0]) and SC.ops_of(T, TORIC, 5, 13) == ops_of(T, TORIC, 5, 13, 0)


def forced_holds_case():
    """toric L = 5 at hbm_width 16 and tile 8: one syndrome, its chains and weights (tests/test_gpu_class_sweep_tiled.py runs the same case)"""
    return random_errors(TORIC, 5, 1, np.random.default_rng([43, 5])), S.SKEW


def test_forced_holds_agree_with_the_cut_twin(T):
    """hbm_width 16 holds 5 generators where the cut plan at width 13 holds 8: another split of the same sum"""
    inf = info(T, TORIC, 5, 16, 8)[1]
    assert (inf["held"], inf["width"], inf["state_bits"]) == (5, 16, 16)
    work = sum(1 << bits(mask) for _, _, _, mask, _, _ in ops_of(T, TORIC, 5, 16, 8))        # live entries an op walks
    print("toric L=5 at width 16: %d entry-ops per partial" % work)
    assert 3e6 < work < 1.2e7                                                   # (6e6: what the twin of this test costs, times 16 classes and 32 assignments)
    chains, w4 = forced_holds_case()
    z, cls = twin(T, TORIC, 5, chains, w4, 16, 8)
    want, wcls = SC.twin(T, TORIC, 5, chains, w4, 13)
    print("max relative difference %.3g" % S.rel(z, want).max())
    assert S.rel(z, want).max() < 1e-12 and np.array_equal(cls, wcls) and np.all(z > 0)


@pytest.mark.parametrize("code,L", [(ROTATED, 13), (ROTATED, 17), (PLANAR, 8)])
def test_all_ones_weights_count_the_group(T, code, L):
    """w = (1, 1, 1, 1): every class weight is 2^rank exactly: sums of equal powers of two"""
    inf = info(T, code, L)[1]
    chains = random_errors(code, L, 1, np.random.default_rng([5, code, L]))
    z, _ = twin(T, code, L, chains, np.ones(4))
    assert inf["rank"] == {PLANAR: 2 * L * (L - 1)}.get(code, L * L - 1) and inf["held"] == 0
    assert np.all(z == 2.0 ** inf["rank"])


def test_twin_is_an_independent_elimination_at_rotated_L13(T):
    """test_class_sweep_cpu.eliminate -- a NumPy array with one axis per open generator, over the oracle's stencils in REVERSED qubit order, 2^16 states
    at most -- under Z-biased noise, two syndromes"""
    code, L = ROTATED, 13
    chains = random_errors(code, L, 2, np.random.default_rng([8, code, L]))
    gens = generators(code, L)
    w4 = ex.biased_w4(0.1, 3.0)
    z, cls = twin(T, code, L, chains, w4)
    assert np.array_equal(cls, classes(code, chains))
    for s, m in enumerate(chains):
        want = np.array([S.eliminate(gens, r, w4) for r in class_chains(code, m)])
        print("rotated 13 syndrome", s, "max relative difference %.3g" % S.rel(z[s], want).max())
        assert S.rel(z[s], want).max() < 1e-12


def test_tile_width_does_not_change_a_bit(T):
    chains = random_errors(ROTATED, 9, 2, np.random.default_rng([44, 9]))
    a, _ = twin(T, ROTATED, 9, chains, S.SKEW, 0, 8)
    b, _ = twin(T, ROTATED, 9, chains, S.SKEW, 0, 13)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(a.view(np.uint64), S.twin(T, ROTATED, 9, chains, S.SKEW)[0].view(np.uint64))


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(T):
    for code, L in [(XZZX, 4), (TORIC, 1), (TORIC, 65), (-1, 3), (4, 3)]:
        assert info(T, code, L)[0] == -1, (code, L)
    for tw in (1, 3, 14, -1, 99):
        rc, _, msg = info(T, XZZX, 3, 0, tw)
        assert rc == -1 and b"tile_width" in msg, (tw, msg)
    for hw, tw in [(10, 0), (12, 13), (25, 0), (-1, 0), (99, 0), (7, 8), (4, 5)]:
        rc, _, msg = info(T, XZZX, 3, hw, tw)
        assert rc == -1 and b"hbm_width" in msg, (hw, tw, msg)
    assert info(T, XZZX, 3, 8, 8)[0] == 0 and info(T, XZZX, 3, 24, 4)[0] == 0 and info(T, XZZX, 3, 4, 4)[0] == 0
    for code, L, hw, frags in [(TORIC, 4, 0, [b"even length"]), (TORIC, 9, 0, [b"37 generators wide", b"held generators", b"width 24"]),
                               (TORIC, 11, 0, [b"45 generators wide"]), (PLANAR, 13, 0, [b"26 generators wide", b"12 held generators leave width 25"]),
                               (ROTATED, 23, 0, [b"26 generators wide", b"12 held generators leave width 26"]), (XZZX, 23, 0, [b"26 generators wide"]),
                               (PLANAR, 14, 0, [b"28 generators wide"]), (ROTATED, 25, 0, [b"28 generators wide"]), (TORIC, 63, 0, [b"held generators"]), (PLANAR, 64, 0, [b"128 generators wide"]),
                               (ROTATED, 63, 0, [b"66 generators wide"]), (TORIC, 7, 16, [b"29 generators wide", b"width 16"]),
                               (ROTATED, 21, 13, [b"24 generators wide", b"12 held generators leave width"])]:
        rc, inf, msg = info(T, code, L, hw)
        print(NAME[code], L, hw, msg)
        assert rc == -4 and all(f in msg for f in frags), (code, L, hw, msg)
    # the entry points of before answer what they answered
    for code, L, frag in [(TORIC, 7, b"29 generators wide"), (PLANAR, 8, b"16 generators wide"), (ROTATED, 13, b"16 generators wide")]:
        rc, _, msg = S.info(T, code, L)
        assert rc == -4 and frag in msg and b"65536 bytes" in msg and b"width 13 at most" in msg
        rc, _, msg = SC.info(T, code, L, 0)
        assert rc == -4 and frag in msg and b"held generators" in msg
    chains, z = np.zeros((1, 9), np.uint8), np.zeros((1, 4))
    call = lambda w, c=chains, out=z, hw=0, tw=0: T.qt_class_sweep_tiled(XZZX, 3, 1, None if c is None else c.ctypes.data_as(_u8p),
                                                                         None if w is None else np.array(w, np.float64).ctypes.data_as(_f64p), hw, tw,
                                                                         None if out is None else out.ctypes.data_as(_f64p), None)
    assert call([1, 1, 1, 1]) == 0
    for bad in ([1, 0, 1, 1], [1, 1, -0.5, 1], [1, 1, 1, np.nan], [np.inf, 1, 1, 1]):
        assert call(bad) == -1, bad
    assert call(None) == -1 and call([1, 1, 1, 1], c=None) == -1 and call([1, 1, 1, 1], out=None) == -1
    assert call([1, 1, 1, 1], tw=3) == -1 and call([1, 1, 1, 1], hw=25) == -1 and call([1, 1, 1, 1], hw=5, tw=6) == -1


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    chains, z, cls = np.zeros((1, 9), np.uint8), np.zeros((1, 4)), np.zeros(1, np.int32)
    big = np.zeros((1, 2 * 13 * 13), np.uint8)
    zp = z.ctypes.data_as(_f64p)
    wp = lambda w: np.array(w, np.float64).ctypes.data_as(_f64p)
    ones = wp([1, 1, 1, 1])
    tiled = lib.qecmc_class_sweep_tiled
    assert tiled(XZZX, 3, 1, None, ones, 0, 0, zp, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert tiled(XZZX, 3, 1, L_.u8(chains), None, 0, 0, zp, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert tiled(XZZX, 3, 1, L_.u8(chains), ones, 0, 0, None, None) == -1 and b"NULL" in lib.qecmc_last_error()
    for bad in ([1, 0, 1, 1], [1, 1, -1, 1], [1, 1, 1, np.nan], [1, np.inf, 1, 1]):
        assert tiled(XZZX, 3, 1, L_.u8(chains), wp(bad), 0, 0, zp, None) == -1 and b"finite and > 0" in lib.qecmc_last_error()
    assert tiled(XZZX, 4, 1, L_.u8(chains), ones, 0, 0, zp, None) == -1 and b"odd L" in lib.qecmc_last_error()
    assert tiled(7, 3, 1, L_.u8(chains), ones, 0, 0, zp, None) == -1 and b"code" in lib.qecmc_last_error()
    for tw in (3, 14, -3):
        assert tiled(XZZX, 3, 1, L_.u8(chains), ones, 0, tw, zp, None) == -1 and b"tile_width" in lib.qecmc_last_error()
    for hw in (10, 25, -3):
        assert tiled(XZZX, 3, 1, L_.u8(chains), ones, hw, 0, zp, None) == -1 and b"hbm_width" in lib.qecmc_last_error()
    assert tiled(TORIC, 4, 1, L_.u8(big), ones, 0, 0, zp, None) == -4 and b"even length" in lib.qecmc_last_error()
    assert tiled(TORIC, 9, 1, L_.u8(big), ones, 0, 0, zp, None) == -4 and b"37 generators wide" in lib.qecmc_last_error()
    assert tiled(TORIC, 7, 1, L_.u8(big), ones, 16, 0, zp, None) == -4 and b"held generators" in lib.qecmc_last_error()
    # the entry points of before still answer -4 at the shapes the tiled sweep adds
    assert lib.qecmc_class_sweep_cut(ROTATED, 13, 1, L_.u8(big), ones, 0, zp, None) == -4 and b"held generators" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep(ROTATED, 13, 1, L_.u8(big), ones, zp, None) == -4 and b"16 generators wide" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep_cut_info(TORIC, 7, 0, None, None, None, None, None, None) == -4
    assert lib.qecmc_abi_version() == 4
    v = [C.c_int32() for _ in range(7)]
    assert lib.qecmc_class_sweep_tiled_info(TORIC, 7, 0, 0, *[C.byref(x) for x in v]) == 0 and [x.value for x in v][:5] == [29, 24, 5, 16, 98]
    assert lib.qecmc_class_sweep_tiled_info(ROTATED, 21, 0, 0, None, None, None, None, None, None, None) == 0
    assert lib.qecmc_class_sweep_tiled_info(TORIC, 9, 0, 0, None, None, None, None, None, None, None) == -4
    # a valid call gets as far as the device lookup: no device, no CPU fallback
    have = L_.device_count() >= 1
    for n in (1, 0):
        assert tiled(XZZX, 3, n, L_.u8(chains), ones, 0, 0, zp, L_.i32(cls)) == (0 if have else -2)
    if not have:
        assert b"no CPU fallback" in lib.qecmc_last_error()
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.class_sweep_tiled("xzzx", chains.reshape(1, 3, 3), np.ones(4))
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.exact_class_probabilities("rotated", np.zeros((1, 13, 13), np.uint8), 0.1, method="tiled")
    with pytest.raises(ValueError, match="four weights"):
        ex.class_sweep_tiled("xzzx", chains.reshape(1, 3, 3), np.ones(3))
    with pytest.raises(L_.QecmcError, match="tile_width"):
        ex.class_sweep_tiled("xzzx", chains.reshape(1, 3, 3), np.ones(4), tile_width=14)
    with pytest.raises(L_.QecmcError, match="hbm_width"):
        ex.exact_class_probabilities("xzzx", chains.reshape(1, 3, 3), 0.1, method="tiled", hbm_width=25)


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_auto_never_answers_tiled(T):
    """resolve_method is what it was: the tiled sweep runs only where it is named, and the refusal of "auto" at its shapes is still the sweep's"""
    import test_enumerate_cpu as E
    for code, L in E.SUPPORTED:
        assert ex.resolve_method(NAME[code], L) == "enumerate" and ex.resolve_method(code, L, "tiled") == "tiled"
    for code, L in [(XZZX, 7), (XZZX, 9), (ROTATED, 7), (ROTATED, 9), (PLANAR, 5), (PLANAR, 6)]:
        assert ex.resolve_method(NAME[code], L) == "sweep"
    for code, L in [(TORIC, 5), (XZZX, 11), (ROTATED, 11), (PLANAR, 7)]:
        assert ex.resolve_method(NAME[code], L) == "cut"
    for code, L in [(TORIC, 4), (TORIC, 7), (PLANAR, 8), (PLANAR, 12), (ROTATED, 13), (ROTATED, 21), (TORIC, 9), (PLANAR, 13), (ROTATED, 23)]:
        assert ex.resolve_method(NAME[code], L) == "sweep" and ex.resolve_method(NAME[code], L, "tiled") == "tiled"
    with pytest.raises(L_.QecmcError, match="16 generators wide.*LDS"):         # the sweep's refusal, before a device is looked for
        ex.exact_class_probabilities("rotated", np.zeros((1, 13, 13), np.uint8), 0.1)
    with pytest.raises(ValueError, match="chunks"):
        ex.exact_class_probabilities("rotated", np.zeros((1, 13, 13), np.uint8), 0.1, method="tiled", chunks=(0, 1))
    with pytest.raises(ValueError, match="device 0"):
        ex.exact_class_probabilities("rotated", np.zeros((1, 13, 13), np.uint8), 0.1, method="tiled", device=1)


# ------------------------------------------------------------------------------------------------------ the sanitizers
def test_tiled_sweep_under_sanitizers():
    """a stand-alone program (its own main) built from class_sweep_tiled.hpp with -fsanitize=address,undefined: tiled plans of every (code, L) up to 13
    and a few beyond, accepted or refused, under several widths; the twin against the cut twin; and the segment table walked tile by tile, as the
    kernel walks it, over NaN-filled memory against the twin bit for bit; run as a child process"""
    run_selftest("sweep_tiled_asan", "class_sweep_tiled_selftest_asan")
