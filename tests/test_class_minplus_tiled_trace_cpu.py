"""A shortest chain of every class on the tiled plans (the traceback of csrc/class_minplus_tiled_trace.hpp), without a GPU: the twins
minplus_tiled_trace_host and minplus_tiled_trace_site_host, compiled by g++ into the host-table test library (qt_class_minplus_tiled_chains, ..._site,
qt_class_minplus_tiled_trace_plan, qt_class_minplus_tiled_trace_pass), and the Python layer around them.

What is pinned: the plan -- forget_words[i] is generator forget_gen[i] of the oracle's table, held and retired generators are the table, each once,
forget_tile and its offsets follow the segment table, the pairs of a pass obey the cap --; the twin against the cut twin byte for byte where the two
plans have one stream; at rotated L = 13, 15 and planar L = 8, the first shapes only this route takes, every chain has the input's syndrome and the
requested class by the oracle and costs what minplus_tiled_host says; on rows with count == 1 three representatives of a syndrome give the same
bytes; forced holds; the tie rule; the zero syndrome; the site twin; refusals by name; the Python layer; the ABI version and N == 0.  Every
comparison is of integers and exact."""
import ctypes as C

import numpy as np
import pytest

import test_class_minplus_cpu as M
import test_class_minplus_site_cpu as MS
import test_class_minplus_tiled_cpu as MT
import test_class_minplus_trace_cpu as TR
import test_class_sweep_tiled_cpu as ST
import test_enumerate_cpu as E
from qecmc import _lib as L_
from qecmc import exact as ex
from qecmc import harness
from test_corrections_cpu import classes, generators, syndromes
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, state_shape
from util_minplus_trace import chain_cost

NAME = M.NAME
UNIT, SPLIT, SPLIT2, COSTS = MT.UNIT, MT.SPLIT, MT.SPLIT2, MT.COSTS
CAP = 2 << 30
INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -4                                    # QECMC_ERR_* (include/qecmc.h)
_u8p, _u32p, _i32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
PREFIX, SITE_PREFIX = b"qecmc_class_minplus_tiled_chains:", b"qecmc_class_minplus_tiled_chains_site:"
nq_of = MT.nq_of


def load_twin():
    """the host-table test library with the tiled traceback's entry points next to every sibling's (tests/test_gpu_class_minplus_tiled_trace.py compares
    the GPU with it)"""
    lib = TR.load_twin()
    MT.load_twin()                                                              # (one CDLL per path: the tiled twins' argtypes on the same object)
    lib.qt_class_minplus_tiled_chains.restype = lib.qt_class_minplus_tiled_chains_site.restype = lib.qt_class_minplus_tiled_trace_plan.restype = C.c_int
    lib.qt_class_minplus_tiled_chains.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _u32p, C.c_int, C.c_int, _u8p, _u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_minplus_tiled_chains_site.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _u8p, C.c_uint64, C.c_int, C.c_int, _u8p, _u32p, _u64p, _i32p, C.c_char_p,
                                                       C.c_int]
    lib.qt_class_minplus_tiled_trace_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, _i32p, _u32p, _u32p, _u32p, C.c_int, _u64p, C.c_char_p, C.c_int]
    lib.qt_class_minplus_tiled_trace_pass.restype = C.c_uint32
    lib.qt_class_minplus_tiled_trace_pass.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def _outputs(code, L, n):
    ncls = 16 if code == TORIC else 4
    return (np.full((n, ncls, nq_of(code, L)), 0xEE, np.uint8), np.full((n, ncls), 77, np.uint32), np.full((n, ncls), 77, np.uint64), np.full(n, 9, np.int32))


def twin_rc(T, code, L, chains, costs, hbm_width=0, tile_width=0):
    """(rc, message, chains uint8[N, ncls, nq], cost, count, cls) of the uniform twin on chains [N, ...]; the outputs start out poisoned"""
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq_of(code, L))
    c = None if costs is None else np.array(costs, np.uint32)
    out, cost, count, cls = _outputs(code, L, len(flat))
    msg = C.create_string_buffer(640)
    rc = T.qt_class_minplus_tiled_chains(code, L, len(flat), flat.ctypes.data_as(_u8p), None if c is None else c.ctypes.data_as(_u32p), hbm_width, tile_width,
                                         out.ctypes.data_as(_u8p), cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), cls.ctypes.data_as(_i32p), msg, 640)
    return rc, msg.value, out, cost, count, cls


def twin(T, code, L, chains, costs, hbm_width=0, tile_width=0):
    rc, msg, out, cost, count, cls = twin_rc(T, code, L, chains, costs, hbm_width, tile_width)
    assert rc == 0, msg
    return out, cost, count, cls


def site_twin_rc(T, code, L, chains, cq, hbm_width=0, tile_width=0, rows=None):
    nq = nq_of(code, L)
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    table = None if cq is None else np.ascontiguousarray(cq, dtype=np.uint8).reshape(-1, nq, 4)
    rows = len(table) if rows is None else rows
    out, cost, count, cls = _outputs(code, L, len(flat))
    msg = C.create_string_buffer(640)
    rc = T.qt_class_minplus_tiled_chains_site(code, L, len(flat), flat.ctypes.data_as(_u8p), None if table is None else table.ctypes.data_as(_u8p), rows, hbm_width,
                                              tile_width, out.ctypes.data_as(_u8p), cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), cls.ctypes.data_as(_i32p),
                                              msg, 640)
    return rc, msg.value, out, cost, count, cls


def site_twin(T, code, L, chains, cq, hbm_width=0, tile_width=0):
    rc, msg, out, cost, count, cls = site_twin_rc(T, code, L, chains, cq, hbm_width, tile_width)
    assert rc == 0, msg
    return out, cost, count, cls


def trace_plan(T, code, L, hbm_width=0, tile_width=0, cap=0):
    """dict(forget_gen int32[n], forget_chains uint8[n, nq], forget_tile uint32[n, 4], seg_forget uint32[segments], n_forget, words_per_tile, W,
    pair_bytes, cap, state_bits, segments, held), or the refusal's message where the plan is refused"""
    _, inf, _ = ST.info(T, code, L, hbm_width, tile_width)
    W, rows = (inf["nq"] + 15) // 16, max(inf["n_gen"], inf["segments"], 1)
    gen, words, tile, seg = np.full(rows, -1, np.int32), np.zeros(rows * W, np.uint32), np.zeros(rows * 4, np.uint32), np.zeros(rows, np.uint32)
    out8, msg = np.zeros(8, np.uint64), C.create_string_buffer(640)
    n = T.qt_class_minplus_tiled_trace_plan(code, L, hbm_width, tile_width, cap, gen.ctypes.data_as(_i32p), words.ctypes.data_as(_u32p), tile.ctypes.data_as(_u32p),
                                            seg.ctypes.data_as(_u32p), rows, out8.ctypes.data_as(_u64p), msg, 640)
    if n < 0:
        return msg.value
    words, q = words[:n * W].reshape(n, W), np.arange(inf["nq"])
    d = dict(zip(("n_forget", "words_per_tile", "W", "pair_bytes", "cap", "state_bits", "segments", "held"), (int(x) for x in out8)))
    d.update(forget_gen=gen[:n], forget_chains=((words[:, q >> 4] >> ((q & 15) * 2).astype(np.uint32)) & 3).astype(np.uint8), forget_tile=tile[:4 * n].reshape(n, 4),
             seg_forget=seg[:d["segments"]])
    return d


# ------------------------------------------------------------------------------------------------------ the plan
# every (code, L, hbm_width, tile_width) the tests of this file and of the GPU file use
PLANS = [(XZZX, 5, 0, 0), (XZZX, 5, 0, 4), (ROTATED, 7, 0, 0), (ROTATED, 7, 0, 5), (ROTATED, 7, 0, 7), (ROTATED, 9, 0, 0), (ROTATED, 9, 0, 8), (PLANAR, 5, 0, 0),
         (TORIC, 3, 13, 0), (TORIC, 3, 0, 6), (TORIC, 3, 8, 4), (TORIC, 5, 13, 0), (ROTATED, 13, 0, 0), (ROTATED, 13, 0, 8), (ROTATED, 13, 0, 13), (ROTATED, 15, 0, 0),
         (PLANAR, 8, 0, 0), (ROTATED, 17, 0, 0), (ROTATED, 21, 0, 0), (XZZX, 21, 0, 0), (PLANAR, 12, 0, 0), (TORIC, 7, 0, 0)]


@pytest.mark.parametrize("code,L,hbm_width,tile_width", PLANS)
def test_plan_names_every_forgets_generator_and_its_place_in_the_decision_block(T, code, L, hbm_width, tile_width):
    gens = generators(code, L)
    _, inf, _ = ST.info(T, code, L, hbm_width, tile_width)
    tp = trace_plan(T, code, L, hbm_width, tile_width)
    tw = tile_width or 11
    print("%s L=%d hbm %d tile %d: width %d, held %d, %d FORGETs, %d words per tile, %d bytes per pair" %
          (NAME[code], L, hbm_width, tile_width, inf["width"], inf["held"], tp["n_forget"], tp["words_per_tile"], tp["pair_bytes"]))
    assert tp["cap"] == CAP and tp["W"] == (inf["nq"] + 15) // 16 and tp["words_per_tile"] == max(1, (1 << (tw - 1)) // 64)
    assert (tp["state_bits"], tp["segments"], tp["held"]) == (max(inf["width"], tw), inf["segments"], inf["held"])
    assert np.array_equal(tp["forget_chains"], gens[tp["forget_gen"]])           # forget_words[i] is generator forget_gen[i] of the oracle's table
    held = ST.held_of(T, code, L, hbm_width, tile_width)[0].tolist()
    assert sorted(held + tp["forget_gen"].tolist()) == list(range(len(gens)))   # held and retired: the table, each exactly once
    # forget_tile and the offsets, from the segment table and the wide stream alone
    ops, off, fi = ST.ops_of(T, code, L, hbm_width, tile_width), 0, 0
    for s, sg in enumerate(ST.segments_of(T, code, L, hbm_width, tile_width)):
        assert tp["seg_forget"][s] == fi
        for kind, slot, top, mask, pairs, qubit in ops[sg["op_first"]:sg["op_first"] + sg["op_count"]]:
            if kind != ST.FORGET:
                continue
            local = bin(sg["tile"] & ((1 << slot) - 1)).count("1")
            assert tp["forget_tile"][fi].tolist() == [sg["tile"], sg["live"] & ~sg["tile"], local, off], (s, fi)
            assert sg["tile"] >> slot & 1 and sg["n_tiles"] == 1 << bin(sg["live"] & ~sg["tile"]).count("1")
            off += sg["n_tiles"] * tp["words_per_tile"]
            fi += 1
    assert fi == tp["n_forget"] and tp["pair_bytes"] == 8 * off <= CAP


def test_bytes_per_pair_of_the_shapes_design_names(T):
    got = {(c, L): trace_plan(T, c, L)["pair_bytes"] for c, L in ((ROTATED, 13), (ROTATED, 17), (ROTATED, 21), (PLANAR, 12), (TORIC, 7))}
    assert got == {(ROTATED, 13): 496896, (ROTATED, 17): 13082880, (ROTATED, 21): 303650944, (PLANAR, 12): 258412928, (TORIC, 7): 77956992}


def test_pairs_of_a_pass_obey_the_workspace_and_the_cap(T):
    P = T.qt_class_minplus_tiled_trace_pass
    for code, L, hbm_width, tile_width in PLANS:
        tp = trace_plan(T, code, L, hbm_width, tile_width)
        units = ST.info(T, code, L, hbm_width, tile_width)[1]["pass_units"]
        for left in (1, 2, 7, 16, 2049, 1 << 20):
            for cap in (0, 1 << 20, 3 * tp["pair_bytes"] + 1):
                n = P(tp["state_bits"], tp["pair_bytes"], left, cap)
                assert n == max(1, min(units, (cap or CAP) // tp["pair_bytes"], left)), (code, L, left, cap)
    assert P(24, 303650944, 16, 0) == 7 and P(16, 496896, 4096, 0) == 2048 and P(16, 496896, 4096, 100 * 496896) == 100
    assert P(24, 1 << 40, 5, 0) == 1                                            # never 0


def test_a_pair_past_the_cap_is_refused_by_name_with_its_bytes(T):
    msg = trace_plan(T, ROTATED, 13, 0, 0, cap=496895)
    assert msg.startswith(PREFIX) and b"496896 bytes" in msg and b"496895" in msg
    assert isinstance(trace_plan(T, ROTATED, 13, 0, 0, cap=496896), dict)


# ------------------------------------------------------------------------------------------------------ the twin is the cut twin where the plans coincide
def same_stream(T, code, L, hbm_width, lds_width):
    """the tiled plan's wide stream and holds are the cut plan's, op for op"""
    import test_class_sweep_cut_cpu as SC
    wide = [(k, s, t, m, sorted(p), q) for k, s, t, m, p, q in ST.ops_of(T, code, L, hbm_width, 0)]
    cut = [(k, s, t, m, sorted(p), q) for k, s, t, m, p, q in SC.ops_of(T, code, L, lds_width)]
    return wide == cut and ST.held_of(T, code, L, hbm_width, 0)[0].tolist() == SC.held_of(T, code, L, lds_width)[0].tolist()


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("code,L,hbm_width,lds_width,n", [(XZZX, 5, 0, 0, 4), (ROTATED, 7, 0, 0, 4), (ROTATED, 9, 0, 0, 3), (PLANAR, 5, 0, 0, 4), (TORIC, 3, 13, 13, 3),
                                                          (TORIC, 5, 13, 13, 1)])
def test_twin_is_the_cut_twin_byte_for_byte(T, code, L, hbm_width, lds_width, n, costs):
    assert same_stream(T, code, L, hbm_width, lds_width)
    chains = MT.chains_of(code, L, n, seed=3)
    got, want = twin(T, code, L, chains, costs, hbm_width), TR.twin(T, code, L, chains, costs, lds_width)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for tile_width in (4, 7):                                                   # (the twin knows nothing of tiles)
        assert all(np.array_equal(a, b) for a, b in zip(twin(T, code, L, chains[:1], costs, hbm_width, tile_width), [w[:1] for w in want]))


# ------------------------------------------------------------------------------------------------------ the shapes only this route takes
def check_properties(code, L, chains, costs, out, cost):
    """every chain of every class: the input's syndrome and the class by the oracle, and the cost the sweep reports"""
    gens = generators(code, L)
    assert out.max() <= 3
    syn = syndromes(code, chains)
    for s in range(len(chains)):
        got = out[s].reshape((out.shape[1],) + state_shape(code, L))
        assert np.array_equal(syndromes(code, got), np.broadcast_to(syn[s], (len(got),) + syn[s].shape)), s
        assert classes(code, got).tolist() == list(range(out.shape[1])), s
        assert [chain_cost(gens, g, costs) for g in got] == cost[s].tolist(), (s, costs)


_first = {}


def first_shapes_case(T, code, L, costs):
    """MT.first_shapes_case's chains and tiled twin, and the traced twin on them, computed once (the GPU file reads the rotated L = 13 rows)"""
    key = (code, L, tuple(costs))
    if key not in _first:
        chains, cost, count, cls = MT.first_shapes_case(T, code, L, costs) if (code, L) != (ROTATED, 15) else \
            ((lambda ch: (ch,) + MT.twin(T, code, L, ch, costs))(MT.few_errors(ROTATED, 15, 1, 12, seed=15)))
        _first[key] = (chains, (cost, count, cls), twin(T, code, L, chains, costs))
    return _first[key]


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("code,L", [(ROTATED, 13), (PLANAR, 8)])
def test_first_shapes_chains_have_the_syndrome_the_class_and_the_cost(T, code, L, costs):
    chains, (want_cost, want_count, want_cls), (out, cost, count, cls) = first_shapes_case(T, code, L, costs)
    assert np.array_equal(cost, want_cost) and np.array_equal(count, want_count) and np.array_equal(cls, want_cls)      # minplus_tiled_host's
    check_properties(code, L, chains, costs, out, cost)


def test_rotated_L15_chains_have_the_syndrome_the_class_and_the_cost(T):
    chains, (want_cost, want_count, want_cls), (out, cost, count, cls) = first_shapes_case(T, ROTATED, 15, SPLIT)
    assert np.array_equal(cost, want_cost) and np.array_equal(count, want_count) and np.array_equal(cls, want_cls)
    check_properties(ROTATED, 15, chains, SPLIT, out, cost)


# ------------------------------------------------------------------------------------------------------ unique rows
def three_representatives(code, L, chains, seed):
    """the chains, the chains times seven generators, and those a logical operator away"""
    gens, rng = generators(code, L), np.random.default_rng([77, code, L, seed])
    moved = chains.copy()
    for s in range(len(moved)):
        for g in rng.integers(len(gens), size=7):
            moved[s] ^= gens[g].reshape(moved[s].shape)
    far = np.stack([E.class_chains(code, m)[(c + 1) % (16 if code == TORIC else 4)].reshape(m.shape) for m, c in zip(moved, classes(code, moved))])
    assert np.array_equal(syndromes(code, far), syndromes(code, chains)) and not np.array_equal(classes(code, far), classes(code, chains))
    return chains, moved, far


UNIQUE = [(ROTATED, 13, 0, 0, 6, 2), (PLANAR, 8, 0, 0, 3, 2), (TORIC, 3, 8, 4, 4, 2)]          # (code, L, hbm_width, tile_width, syndromes, errors each)


@pytest.mark.parametrize("code,L,hbm_width,tile_width,n,k", UNIQUE)
def test_three_representatives_give_the_same_bytes_on_unique_rows(T, code, L, hbm_width, tile_width, n, k):
    reps = three_representatives(code, L, MT.few_errors(code, L, n, k, seed=5), 5)
    runs = [twin(T, code, L, r, UNIT, hbm_width, tile_width) for r in reps]
    unique = runs[0][2] == 1
    print(NAME[code], L, "unique rows:", int(unique.sum()), "of", unique.size)
    assert unique.sum() >= 4
    for out, cost, count, cls in runs[1:]:
        assert np.array_equal(cost, runs[0][1]) and np.array_equal(count, runs[0][2])
        assert np.array_equal(out[unique], runs[0][0][unique])


def test_forced_holds_agree_with_no_holds(T):
    chains = np.concatenate([MT.chains_of(TORIC, 3, 2, seed=6), MT.few_errors(TORIC, 3, 3, 2, seed=6)])
    held, free = twin(T, TORIC, 3, chains, UNIT, 8, 4), twin(T, TORIC, 3, chains, UNIT, 13, 0)
    assert trace_plan(T, TORIC, 3, 8, 4)["held"] > 0 == trace_plan(T, TORIC, 3, 13, 0)["held"]
    assert all(np.array_equal(a, b) for a, b in zip(held[1:], free[1:]))        # cost, count, class
    unique = free[2] == 1
    assert unique.sum() >= 4 and np.array_equal(held[0][unique], free[0][unique])
    check_properties(TORIC, 3, chains, UNIT, held[0], held[1])


# ------------------------------------------------------------------------------------------------------ the tie rule and the zero syndrome
@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 13, 0, 0), (TORIC, 3, 8, 4), (PLANAR, 8, 0, 0)])
def test_all_zero_costs_return_the_class_representative(T, code, L, hbm_width, tile_width):
    chains = MT.chains_of(code, L, 1, seed=7)
    out, cost, count, cls = twin(T, code, L, chains, (0, 0, 0, 0), hbm_width, tile_width)
    assert not cost.any()
    want = np.stack([r.ravel() for r in E.class_chains(code, chains[0])])
    cells = harness._qubit_cells(code, L).ravel()
    assert np.array_equal(out[0][:, cells], want[:, cells])                     # nothing is strictly cheaper: no generator is applied


@pytest.mark.parametrize("code,L", [(ROTATED, 13), (PLANAR, 8)])
def test_the_zero_syndrome_gives_the_identity_for_class_0(T, code, L):
    out, cost, count, cls = twin(T, code, L, np.zeros((1,) + state_shape(code, L), np.uint8), UNIT)
    assert cls[0] == 0 and cost[0, 0] == 0 and count[0, 0] == 1 and not out[0, 0].any()
    check_properties(code, L, np.zeros((1,) + state_shape(code, L), np.uint8), UNIT, out, cost)


# ------------------------------------------------------------------------------------------------------ the site twin
@pytest.mark.parametrize("costs", [UNIT, (1, 0, 2, 3)])
@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4), (ROTATED, 13, 0, 0)])
def test_site_constant_rows_equal_the_uniform_twin(T, code, L, hbm_width, tile_width, costs):
    chains = MT.chains_of(code, L, 2, seed=8)
    cq = np.broadcast_to(np.array(costs, np.uint8), (1, nq_of(code, L), 4))
    got, want = site_twin(T, code, L, chains, cq, hbm_width, tile_width), twin(T, code, L, chains, costs, hbm_width, tile_width)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4)])
def test_site_rows_travel_with_their_syndromes(T, code, L, hbm_width, tile_width):
    n = 4
    chains, cq = MT.chains_of(code, L, n, seed=9), MS.tables_of(code, L, n, "bytes", seed=9)
    out, cost, count, cls = site_twin(T, code, L, chains, cq, hbm_width, tile_width)
    MS.check_chains(code, L, chains, cq, out, cost)
    want = MT.site_twin(T, code, L, chains, cq, hbm_width, tile_width)
    assert np.array_equal(cost, want[0]) and np.array_equal(count, want[1]) and np.array_equal(cls, want[2])
    for s in range(n):                                                          # row s alone, as one table
        one = site_twin(T, code, L, chains[s:s + 1], cq[s:s + 1], hbm_width, tile_width)
        assert all(np.array_equal(a[0], b[s]) for a, b in zip(one, (out, cost, count, cls)))
    cut = MS.twin(T, code, L, chains, cq) if hbm_width == 0 else None           # (nothing held: the cut plan's stream)
    assert cut is None or all(np.array_equal(a, b) for a, b in zip((out, cost, count, cls), cut))


def test_site_twin_does_not_read_the_planar_codes_unused_cells(T):
    chains, cq = MT.chains_of(PLANAR, 5, 3, seed=10), MS.tables_of(PLANAR, 5, 3, "bytes", seed=10)
    poisoned = cq.copy()
    poisoned[:, ~harness._qubit_cells(PLANAR, 5).ravel()] = 255
    got, want = site_twin(T, PLANAR, 5, chains, poisoned), site_twin(T, PLANAR, 5, chains, cq)
    cells = harness._qubit_cells(PLANAR, 5).ravel()
    assert np.array_equal(got[0][:, :, cells], want[0][:, :, cells]) and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))


def test_llr_site_costs_at_rotated_L13(T):
    rng = np.random.default_rng(11)
    p = rng.uniform(0.01, 0.2, size=(13, 13))
    cq = ex.llr_site_costs(ex.depolarizing_site_w4(p), 2.0)
    assert cq.max() <= 255 and len(np.unique(cq)) > 4
    chains = MT.chains_of(ROTATED, 13, 1, seed=11)
    out, cost, count, cls = site_twin(T, ROTATED, 13, chains, cq[None])
    MS.check_chains(ROTATED, 13, chains, cq.reshape(1, -1, 4), out, cost)
    assert np.array_equal(cost, MT.site_twin(T, ROTATED, 13, chains, cq[None])[0])


# ------------------------------------------------------------------------------------------------------ refusals
def test_the_twin_refuses_by_name(T):
    chains = MT.chains_of(ROTATED, 13, 1)
    for kw, code_, want in [(dict(tile_width=3), INVALID, b"tile_width=3"), (dict(tile_width=14), INVALID, b"tile_width=14"),
                            (dict(hbm_width=25), INVALID, b"hbm_width=25"), (dict(hbm_width=10), INVALID, b"hbm_width=10")]:
        rc, msg = twin_rc(T, ROTATED, 13, chains, UNIT, **kw)[:2]
        assert rc == code_ and msg.startswith(PREFIX) and want in msg, msg
        rc, msg = site_twin_rc(T, ROTATED, 13, chains, np.ones((1, 169, 4), np.uint8), **kw)[:2]
        assert rc == code_ and msg.startswith(SITE_PREFIX) and want in msg, msg
    rc, msg = twin_rc(T, TORIC, 4, np.zeros((1, 2, 4, 4), np.uint8), UNIT)[:2]
    assert rc == UNSUPPORTED and msg.startswith(PREFIX), msg             # no class move at even L
    rc, msg = twin_rc(T, TORIC, 9, np.zeros((1, 2, 9, 9), np.uint8), UNIT)[:2]
    assert rc == UNSUPPORTED and msg.startswith(PREFIX) and b"generators wide" in msg, msg
    rc, msg = twin_rc(T, ROTATED, 13, chains, (0, 1, 256, 1))[:2]
    assert rc == INVALID and msg.startswith(PREFIX), msg                 # a cost above 255
    rc, msg = twin_rc(T, ROTATED, 21, np.zeros((1, 21, 21), np.uint8), (0, 149, 1, 1))[:2]
    assert rc == UNSUPPORTED and msg.startswith(PREFIX) and b"441 * 149" in msg, msg      # the cost range, per call
    rc, msg = site_twin_rc(T, ROTATED, 21, np.zeros((1, 21, 21), np.uint8), np.full((1, 441, 4), 149, np.uint8))[:2]
    assert rc == UNSUPPORTED and msg.startswith(SITE_PREFIX) and b"cq row 0" in msg, msg
    rc, msg = site_twin_rc(T, ROTATED, 13, MT.chains_of(ROTATED, 13, 3), np.ones((2, 169, 4), np.uint8))[:2]
    assert rc == INVALID and msg.startswith(SITE_PREFIX) and b"cq_rows=2" in msg, msg
    rc, msg = twin_rc(T, ROTATED, 13, chains, None)[:2]
    assert rc == INVALID and msg == PREFIX + b" NULL buffer"
    rc, msg = site_twin_rc(T, ROTATED, 13, chains, None, rows=1)[:2]
    assert rc == INVALID and msg == SITE_PREFIX + b" NULL buffer"


def test_the_library_refuses_on_the_host_and_n_0_and_the_abi(T):
    lib = L_.lib()
    assert lib.qecmc_abi_version() == 4
    chains, c = np.zeros((1, 169), np.uint8), np.array(UNIT, np.uint32)
    out, cost, count, cls = _outputs(ROTATED, 13, 1)

    def call(code, L, n, costs, hbm_width=0, tile_width=0, chain_out=out):
        return lib.qecmc_class_minplus_tiled_chains(code, L, n, L_.u8(chains), None if costs is None else costs.ctypes.data_as(_u32p), hbm_width, tile_width,
                                                    None if chain_out is None else L_.u8(chain_out), cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), L_.i32(cls))
    for args, rc_want, want in [((ROTATED, 13, 1, c, 0, 3), INVALID, "tile_width=3"), ((ROTATED, 13, 1, c, 25, 0), INVALID, "hbm_width=25"),
                                ((TORIC, 4, 1, c), UNSUPPORTED, ""), ((ROTATED, 13, 1, None), INVALID, "NULL buffer"),
                                ((ROTATED, 13, 1, c, 0, 0, None), INVALID, "NULL buffer"), ((ROTATED, 13, 1 << 32, c), INVALID, "exceed 32 bits"),
                                ((ROTATED, 13, 1, np.array((0, 1, 300, 1), np.uint32)), INVALID, ""),
                                ((ROTATED, 21, 1, np.array((0, 149, 1, 1), np.uint32)), UNSUPPORTED, "441 * 149")]:
        assert call(*args) == rc_want, args                                     # before a device is looked for: this machine may have none
        msg = lib.qecmc_last_error().decode()
        assert msg.startswith(PREFIX.decode()) and want in msg, msg
    cq = np.ones((1, 169, 4), np.uint8)
    site = lib.qecmc_class_minplus_tiled_chains_site
    assert site(ROTATED, 13, 1, L_.u8(chains), None, 1, 0, 0, L_.u8(out), None, None, None) == INVALID
    assert lib.qecmc_last_error().decode() == SITE_PREFIX.decode() + " NULL buffer"
    assert site(ROTATED, 13, 3, L_.u8(np.zeros((3, 169), np.uint8)), L_.u8(cq), 2, 0, 0, L_.u8(out), None, None, None) == INVALID
    assert lib.qecmc_last_error().decode().startswith(SITE_PREFIX.decode()) and "cq_rows=2" in lib.qecmc_last_error().decode()
    # N == 0 succeeds where a device is there, and asks for one where none is: every refusal above came first
    rc = call(ROTATED, 13, 0, c)
    assert rc == (0 if L_.lib().qecmc_device_count() > 0 else NO_DEVICE)


# ------------------------------------------------------------------------------------------------------ the Python layer and the harness
class FakeLib:
    """qecmc_class_minplus_tiled_chains(_site) and the info call answered by the twin: the Python layer around them, without a device"""
    def __init__(self, T):
        self.T, self.real, self.calls = T, L_.lib(), []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def qecmc_class_minplus_tiled_chains(self, code, L, n, chains, cost, hbm_width, tile_width, chain_out, cost_out, count_out, cls):
        self.calls.append(("uniform", code, L, n, hbm_width, tile_width))
        return self.T.qt_class_minplus_tiled_chains(code, L, n, C.cast(chains, _u8p), cost, hbm_width, tile_width, C.cast(chain_out, _u8p), cost_out, count_out,
                                                    C.cast(cls, _i32p), None, 0)

    def qecmc_class_minplus_tiled_chains_site(self, code, L, n, chains, cq, rows, hbm_width, tile_width, chain_out, cost_out, count_out, cls):
        self.calls.append(("site", code, L, n, hbm_width, tile_width))
        return self.T.qt_class_minplus_tiled_chains_site(code, L, n, C.cast(chains, _u8p), C.cast(cq, _u8p), rows, hbm_width, tile_width, C.cast(chain_out, _u8p),
                                                         cost_out, count_out, C.cast(cls, _i32p), None, 0)


def test_python_layer_shapes_keys_and_routes(T, monkeypatch):
    fake = FakeLib(T)
    monkeypatch.setattr(L_, "lib", lambda: fake)
    chains = MT.chains_of(ROTATED, 7, 3, seed=12)
    r = ex.shortest_chains_tiled("rotated", chains, SPLIT, tile_width=5)
    out, cost, count, cls = twin(T, ROTATED, 7, chains, SPLIT, 0, 5)
    assert set(r) == {"chains", "cost", "count", "saturated", "unique", "cls", "width", "held", "segments"}
    assert r["chains"].shape == (3, 4, 7, 7) and r["chains"].dtype == np.uint8 and np.array_equal(r["chains"].reshape(3, 4, -1), out)
    assert np.array_equal(r["cost"], cost) and np.array_equal(r["count"], count) and np.array_equal(r["cls"], cls) and np.array_equal(r["unique"], count == 1)
    assert r["segments"] == ST.info(T, ROTATED, 7, 0, 5)[1]["segments"] and r["held"] == 0
    cq = MS.tables_of(ROTATED, 7, 3, "bytes", seed=12)
    rs = ex.shortest_chains_tiled_site("rotated", chains, cq.reshape(3, 7, 7, 4), tile_width=5)
    assert np.array_equal(rs["chains"].reshape(3, 4, -1), site_twin(T, ROTATED, 7, chains, cq, 0, 5)[0]) and set(rs) == set(r)
    m = ex.min_weight_corrections("rotated", chains, SPLIT, method="tiled", tile_width=5)
    target = ex._rank_classes(cost, count)
    assert np.array_equal(m["target"], target) and np.array_equal(m["correction"].reshape(3, -1), out[np.arange(3), target])
    assert np.array_equal(m["weight"], cost[np.arange(3), target])
    ms = ex.min_weight_corrections_site("rotated", chains, cq.reshape(3, 7, 7, 4), method="tiled", tile_width=5)
    assert np.array_equal(ms["correction"], rs["chains"][np.arange(3), ms["target"]])
    assert [c[0] for c in fake.calls] == ["uniform", "site", "uniform", "site"] and all(c[-1] == 5 for c in fake.calls)
    # a width of the other route is refused by name, as min_weight_classes refuses it; the default stays the cut route
    with pytest.raises(ValueError, match="lds_width belongs to method='cut'"):
        ex.min_weight_corrections("rotated", chains, method="tiled", lds_width=13)
    with pytest.raises(ValueError, match="hbm_width and tile_width belong to method='tiled'"):
        ex.min_weight_corrections("rotated", chains, tile_width=5)
    with pytest.raises(ValueError, match="hbm_width and tile_width belong to method='tiled'"):
        ex.min_weight_corrections_site("rotated", chains, cq.reshape(3, 7, 7, 4), hbm_width=20)
    with pytest.raises(ValueError, match="method='auto'"):
        ex.min_weight_corrections("rotated", chains, method="auto")
    with pytest.raises(ValueError, match="costs="):
        ex.shortest_chains_tiled("rotated", chains, (0, 1, 1))
    import qecmc
    assert qecmc.shortest_chains_tiled is ex.shortest_chains_tiled and qecmc.shortest_chains_tiled_site is ex.shortest_chains_tiled_site


def test_harness_takes_shortest_tiled_only_on_the_tiled_min_weight_route():
    base = dict(code="rotated", size=13, p_error=0.05)
    for method in ("PTEQ", "exact"):
        with pytest.raises(ValueError, match="params\\['correction'\\]='shortest_tiled' is built for method min_weight, not " + method):
            harness._correction_route(dict(base, method=method, correction="shortest_tiled", exact_method="tiled"), method)
    for exact_method in (None, "auto", "cut"):
        params = dict(base, method="min_weight", correction="shortest_tiled")
        if exact_method:
            params["exact_method"] = exact_method
        with pytest.raises(ValueError, match="params\\['correction'\\]='shortest_tiled' is built for params\\['exact_method'\\]='tiled', not"):
            harness._correction_route(params, "min_weight")
        with pytest.raises(ValueError, match="shortest_tiled' is built for params\\['exact_method'\\]='tiled'"):
            harness.decode_syndromes(params, np.zeros((1, 14, 14), np.uint8), corrections=True)
    assert harness._correction_route(dict(base, method="min_weight", exact_method="tiled", correction="shortest_tiled"), "min_weight") == "shortest_tiled"
    with pytest.raises(ValueError, match="correction'\\]='shortest' is not built for params\\['exact_method'\\]='tiled'.*no traceback"):
        harness._correction_route(dict(base, method="min_weight", exact_method="tiled", correction="shortest"), "min_weight")
    with pytest.raises(ValueError, match="params\\['correction'\\]='longest'"):
        harness._correction_route(dict(base, method="min_weight", correction="longest"), "min_weight")
