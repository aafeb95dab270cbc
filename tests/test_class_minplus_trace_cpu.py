"""A shortest chain of every class (the traceback of csrc/class_minplus_trace.hpp), without a GPU: the twin, compiled by g++ into the host-table test
library (qt_class_minplus_chains, qt_class_minplus_trace_plan, qt_class_minplus_trace_group), and the Python layer around it.

What is pinned: the trace plan against the oracle's generator table and the op stream (forget_words[i] is generator forget_gen[i], and the XOR of the
Paulis the CLOSEs name for its slot); held and retired generators are the table, each once; the launch group bounds the decision workspace.  Every
traced chain has the input's syndrome and the requested class by the oracle, and costs what the sweep says; cost and count are qt_class_minplus's.
On rows with count == 1 the chain is the argmin of a brute force over the group (L = 3) and the same from three representatives of the syndrome.
The tie rule: all-zero costs return the class representative itself.  Held generators change costs and classes of no chain.  Refusals by name; the
Python layer; the sanitizers.  Every comparison is integer and exact."""
import ctypes as C

import numpy as np
import pytest

import test_class_minplus_cpu as M
import test_class_sweep_cut_cpu as SC
import test_enumerate_cpu as E
from hostlib import run_selftest
from qecmc import _lib as L_
from qecmc import exact as ex
from test_corrections_cpu import classes, generators, syndromes
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_minplus_trace import brute_force_argmin, chain_cost, coset, qubit_cells

NAME = M.NAME
UNIT, ALPHA3, MIXED, COSTS = M.UNIT, M.ALPHA3, M.MIXED, M.COSTS
INTRO, CLOSE, FORGET = SC.INTRO, SC.CLOSE, SC.FORGET
WORKSPACE = 256 << 20
_u8p, _u32p, _i32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)


def load_twin():
    """the host-table test library with the traceback's entry points (tests/test_gpu_class_minplus_trace.py compares the GPU with it)"""
    lib = M.load_twin()
    lib.qt_class_minplus_chains.restype = C.c_int
    lib.qt_class_minplus_chains.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _u32p, C.c_int, _u8p, _u32p, _u64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_minplus_trace_plan.restype = C.c_int
    lib.qt_class_minplus_trace_plan.argtypes = [C.c_int, C.c_int, C.c_int, _i32p, _u32p, C.c_int, _i32p]
    lib.qt_class_minplus_trace_group.restype = C.c_uint32
    lib.qt_class_minplus_trace_group.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint64, _u64p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def twin_rc(T, code, L, chains, costs, lds_width=0):
    """(rc, message, chains uint8[N, ncls, nq], cost uint32[N, ncls], count uint64[N, ncls], cls int32[N]) of the host twin on chains [N, ...]; the
    outputs start out poisoned"""
    nq = int(np.prod(state_shape(code, L))) if 2 <= L <= 64 else 1
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    c = np.ascontiguousarray(costs, dtype=np.uint32)
    ncls = 16 if code == TORIC else 4
    out = np.full((len(flat), ncls, nq), 0xEE, np.uint8)
    cost, count, cls = np.full((len(flat), ncls), 77, np.uint32), np.full((len(flat), ncls), 77, np.uint64), np.full(len(flat), 9, np.int32)
    msg = C.create_string_buffer(640)
    rc = T.qt_class_minplus_chains(code, L, len(flat), flat.ctypes.data_as(_u8p), c.ctypes.data_as(_u32p), lds_width, out.ctypes.data_as(_u8p),
                                   cost.ctypes.data_as(_u32p), count.ctypes.data_as(_u64p), cls.ctypes.data_as(_i32p), msg, 640)
    return rc, msg.value, out, cost, count, cls


def twin(T, code, L, chains, costs, lds_width=0):
    rc, msg, out, cost, count, cls = twin_rc(T, code, L, chains, costs, lds_width)
    assert rc == 0, msg
    return out, cost, count, cls


def trace_plan(T, code, L, lds_width):
    """(forget_gen int32[n_forget], the retired generators as byte chains uint8[n_forget, nq], dict(n_forget, words_per_forget, W, pair_bytes))"""
    _, inf, _ = SC.info(T, code, L, lds_width)
    W = (inf["nq"] + 15) // 16
    gen, words, out4 = np.full(inf["n_gen"], -1, np.int32), np.zeros(inf["n_gen"] * W, np.uint32), np.zeros(4, np.int32)
    n = T.qt_class_minplus_trace_plan(code, L, lds_width, gen.ctypes.data_as(_i32p), words.ctypes.data_as(_u32p), words.size, out4.ctypes.data_as(_i32p))
    assert n == inf["n_gen"] - inf["held"], (n, inf)
    words = words[:n * W].reshape(n, W)
    q = np.arange(inf["nq"])
    return gen[:n], ((words[:, q >> 4] >> ((q & 15) * 2).astype(np.uint32)) & 3).astype(np.uint8), dict(zip(("n_forget", "words_per_forget", "W", "pair_bytes"), out4.tolist()))


def low_weight_errors(code, L, n, rng, k=2):
    """n errors of at most k Paulis each, on cells that hold a qubit"""
    cells = np.flatnonzero(qubit_cells(generators(code, L)))
    m = np.zeros((n, int(np.prod(state_shape(code, L)))), np.uint8)
    for row in m:
        where = rng.choice(cells, size=int(rng.integers(1, k + 1)), replace=False)
        row[where] = rng.integers(1, 4, size=len(where), dtype=np.uint8)
    return m.reshape((n,) + state_shape(code, L))


# ------------------------------------------------------------------------------------------------------ the plan
PLANS = [(ROTATED, 3, 0), (ROTATED, 5, 0), (ROTATED, 5, 5), (XZZX, 5, 6), (PLANAR, 3, 3), (PLANAR, 4, 0), (TORIC, 3, 0), (TORIC, 3, 6), (TORIC, 5, 0), (ROTATED, 11, 0),
         (PLANAR, 7, 0)]


@pytest.mark.parametrize("code,L,lds_width", PLANS)
def test_trace_plan_names_the_generator_every_forget_retires(T, code, L, lds_width):
    gens = generators(code, L)
    _, inf, _ = SC.info(T, code, L, lds_width)
    forget_gen, forget_chains, tp = trace_plan(T, code, L, lds_width)
    print("%s L=%d lds_width %d: width %d, held %d, %d FORGETs, %d words each, %d bytes per pair" %
          (NAME[code], L, lds_width, inf["width"], inf["held"], tp["n_forget"], tp["words_per_forget"], tp["pair_bytes"]))
    assert tp["words_per_forget"] == max(1, (1 << (inf["width"] - 1)) // 64) and tp["pair_bytes"] == tp["n_forget"] * tp["words_per_forget"] * 8
    assert tp["W"] == (inf["nq"] + 15) // 16
    assert np.array_equal(forget_chains, gens[forget_gen])                      # forget_words[i] is generator forget_gen[i] of the oracle's table
    held = SC.held_of(T, code, L, lds_width)[0].tolist()
    assert sorted(held + forget_gen.tolist()) == list(range(len(gens)))         # held and retired: the table, each exactly once
    # ... and the XOR of the Paulis the CLOSEs name for the slot between its INTRO and its FORGET
    live, fi = {}, 0
    for kind, slot, top, mask, pairs, qubit in SC.ops_of(T, code, L, lds_width):
        if kind == INTRO:
            live[slot] = np.zeros(gens.shape[1], np.uint8)
        elif kind == CLOSE:
            for s, pauli in pairs:
                live[s][qubit] ^= pauli
        else:
            assert np.array_equal(live.pop(slot), forget_chains[fi]), fi
            fi += 1
    assert fi == tp["n_forget"] and not live


def test_launch_group_bounds_the_decision_workspace(T):
    ws = C.c_uint64()
    assert T.qt_class_minplus_trace_group(1, 4, 0, 8, C.byref(ws)) == 1 and ws.value == WORKSPACE
    for code, L, lds_width in PLANS:
        _, inf, _ = SC.info(T, code, L, lds_width)
        tp = trace_plan(T, code, L, lds_width)[2]
        for n in (0, 1, 2, 40, 1000, 5000, 1 << 32):
            group = T.qt_class_minplus_trace_group(n, inf["ncls"], inf["held"], tp["pair_bytes"], None)
            cut = T.qt_class_sweep_cut_group(n, inf["ncls"], inf["held"])
            assert 1 <= group <= cut and group <= max(n, 1)
            assert group * inf["ncls"] * tp["pair_bytes"] <= WORKSPACE
            assert group == cut or (group + 1) * inf["ncls"] * tp["pair_bytes"] > WORKSPACE         # no smaller than the bound asks
    tp = trace_plan(T, ROTATED, 11, 0)[2]
    assert tp["pair_bytes"] == 120 * 1024 and T.qt_class_minplus_trace_group(5000, 4, 0, tp["pair_bytes"], None) == WORKSPACE // (4 * 120 * 1024) < 1024
    assert T.qt_class_minplus_trace_group(7, 16, 0, 1 << 40, None) == 1         # never 0
    assert T.qt_class_minplus_trace_group(7, 16, 0, 0, None) == 7


# ------------------------------------------------------------------------------------------------------ the properties of the twin's chains
def check_properties(T, code, L, chains, costs, lds_width=0):
    """every chain of every class: the input's syndrome and the class by the oracle, the cost the sweep reports; cost and count qt_class_minplus's"""
    gens = generators(code, L)
    out, cost, count, cls = twin(T, code, L, chains, costs, lds_width)
    want_cost, want_count, want_cls = M.twin(T, code, L, chains, costs, lds_width)
    assert np.array_equal(cost, want_cost) and np.array_equal(count, want_count) and np.array_equal(cls, want_cls)
    assert out.max() <= 3
    syn = syndromes(code, chains)
    for s in range(len(chains)):
        got = out[s].reshape((out.shape[1],) + state_shape(code, L))
        assert np.array_equal(syndromes(code, got), np.broadcast_to(syn[s], (len(got),) + syn[s].shape)), s
        assert classes(code, got).tolist() == list(range(out.shape[1])), s
        assert [chain_cost(gens, g, costs) for g in got] == cost[s].tolist(), (s, costs)
    return out, cost, count, cls


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("code,L,n", [(ROTATED, 3, 12), (ROTATED, 5, 9), (ROTATED, 7, 6), (XZZX, 5, 9), (PLANAR, 3, 12), (PLANAR, 4, 9), (PLANAR, 5, 6), (TORIC, 3, 6)])
def test_chains_have_the_syndrome_the_class_and_the_cost(T, code, L, n, costs):
    check_properties(T, code, L, random_errors(code, L, n, np.random.default_rng([71, code, L])), costs)


@pytest.mark.parametrize("costs", COSTS)
def test_chains_at_toric_L5(T, costs):
    """one syndrome: the twin sweeps 16 * 2^8 state vectors for it"""
    check_properties(T, TORIC, 5, random_errors(TORIC, 5, 2, np.random.default_rng([72]))[1:], costs)


# ------------------------------------------------------------------------------------------------------ unique rows
@pytest.mark.parametrize("code", [TORIC, PLANAR, XZZX, ROTATED])
def test_unique_rows_are_the_argmin_of_a_brute_force_at_L3(T, code):
    gens = generators(code, 3)
    chains = low_weight_errors(code, 3, 2 if code == TORIC else 8, np.random.default_rng([73, code]))
    traced = [twin(T, code, 3, chains, costs) for costs in COSTS]
    compared = 0
    for s in range(len(chains)):
        for c, rep in enumerate(E.class_chains(code, chains[s])):
            group = coset(gens, rep)                                            # once for the three cost vectors
            for costs, (out, cost, count, cls) in zip(COSTS, traced):
                least, n_best, best = brute_force_argmin(gens, rep, costs, group)
                assert (int(cost[s, c]), int(count[s, c])) == (least, n_best)
                assert any(np.array_equal(out[s, c], b) for b in best)          # tied or not, it is one of the shortest
                if count[s, c] == 1:
                    assert np.array_equal(out[s, c], best[0])
                    compared += 1
    print(NAME[code], "unique rows compared with the brute force:", compared)
    assert compared >= 10


@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 5, 0), (XZZX, 5, 6), (PLANAR, 4, 0), (TORIC, 3, 8)])
def test_three_representatives_give_the_same_chain_on_unique_rows(T, code, L, lds_width):
    """the chain, the chain times seven generators, and that a logical operator away: where count == 1 the chain is a function of the syndrome"""
    chains = low_weight_errors(code, L, 8, np.random.default_rng([74, code, L]))
    gens, rng = generators(code, L), np.random.default_rng([75, code, L])
    moved = chains.copy()
    for s in range(len(moved)):
        for g in rng.integers(len(gens), size=7):
            moved[s] ^= gens[g].reshape(moved[s].shape)
    compared = 0
    for costs in COSTS:
        out, cost, count, cls = twin(T, code, L, chains, costs, lds_width)
        ncls = cost.shape[1]
        other = np.stack([E.class_chains(code, m)[(c + 1) % ncls].reshape(m.shape) for m, c in zip(moved, cls)])
        for again in (moved, other):
            out2, cost2, count2, _ = twin(T, code, L, again, costs, lds_width)
            assert np.array_equal(cost2, cost) and np.array_equal(count2, count)
            unique = count == 1
            assert np.array_equal(out2[unique], out[unique])
            compared += int(unique.sum())
    print(NAME[code], L, "unique rows compared:", compared)
    assert compared >= 10


# ------------------------------------------------------------------------------------------------------ the tie rule
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 5, 0), (PLANAR, 4, 0), (TORIC, 3, 0), (TORIC, 3, 6), (XZZX, 5, 6)])
def test_all_zero_costs_return_the_class_representative(T, code, L, lds_width):
    """every decision ties, so no generator is applied and h* = 0: the chain of class c is the representative the sweep starts from -- the input times
    the logical operators at position 0, which is the input itself for its own class"""
    chains = random_errors(code, L, 12, np.random.default_rng([76, code, L]))
    out, cost, count, cls = twin(T, code, L, chains, (0, 0, 0, 0), lds_width)
    assert np.all(cost == 0)
    flat = chains.reshape(len(chains), -1)
    moves, shared = {}, 0
    for s in range(len(chains)):
        assert np.array_equal(out[s, cls[s]], flat[s])
        reps = out[s].reshape((out.shape[1],) + state_shape(code, L))
        assert classes(code, reps).tolist() == list(range(out.shape[1]))
        syn = syndromes(code, chains[s:s + 1])[0]
        assert all(np.array_equal(row, syn) for row in syndromes(code, reps))
        # the move from class a to class c is the same product of logical operators whatever the chain: no generator rides on it
        move = out[s] ^ flat[s]
        shared += int(cls[s]) in moves
        assert np.array_equal(moves.setdefault(int(cls[s]), move), move)
    assert shared >= 1


def test_the_zero_syndrome_gives_the_identity_for_class_0(T):
    for code, L in [(ROTATED, 5), (XZZX, 5), (PLANAR, 4), (TORIC, 3), (TORIC, 5)]:
        zero = np.zeros((1,) + state_shape(code, L), np.uint8)
        out, cost, count, cls = twin(T, code, L, zero, UNIT)
        own = int(cls[0])
        assert own == int(classes(code, zero)[0]) and cost[0, own] == 0 and count[0, own] == 1 and not out[0, own].any()
        assert own == 0


# ------------------------------------------------------------------------------------------------------ held generators
def test_held_generators_change_no_cost_and_no_class(T):
    chains = random_errors(TORIC, 3, 6, np.random.default_rng([77]))
    assert SC.info(T, TORIC, 3, 13)[1]["held"] == 0 and SC.info(T, TORIC, 3, 6)[1]["held"] == 7
    for costs in COSTS:
        wide = check_properties(T, TORIC, 3, chains, costs, 13)
        narrow = check_properties(T, TORIC, 3, chains, costs, 6)
        assert np.array_equal(wide[1], narrow[1]) and np.array_equal(wide[2], narrow[2]) and np.array_equal(wide[3], narrow[3])
        unique = wide[2] == 1
        assert np.array_equal(wide[0][unique], narrow[0][unique])               # (tied rows need not be byte-equal)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(T):
    for code, L, costs, w, want, frags in M.REFUSED:
        rc, msg, out, _, _, _ = twin_rc(T, code, L, np.zeros((1, int(np.prod(state_shape(code, L)))), np.uint8), costs, w)
        print(NAME[code], L, costs, w, msg)
        assert rc == want and msg.startswith(b"qecmc_class_minplus_chains:") and all(f in msg for f in frags), (code, L, w, msg)
        assert np.all(out == 0xEE)
    assert twin_rc(T, ROTATED, 3, np.zeros((1, 9), np.uint8), (255, 255, 255, 255))[0] == 0
    assert T.qt_class_minplus_chains(ROTATED, 3, 1, None, None, 0, None, None, None, None, None, 0) == -1
    # cost_out, count_out and cls are nullable
    chains, c = np.zeros((1, 9), np.uint8), np.array(UNIT, np.uint32)
    out = np.full((1, 4, 9), 0xEE, np.uint8)
    assert T.qt_class_minplus_chains(ROTATED, 3, 1, chains.ctypes.data_as(_u8p), c.ctypes.data_as(_u32p), 0, out.ctypes.data_as(_u8p), None, None, None, None, 0) == 0
    assert out.max() <= 3 and not out[0, 0].any()


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    assert lib.qecmc_abi_version() == 4
    big = np.zeros((1, 2 * 13 * 13), np.uint8)
    out = np.zeros((1, 16, 2 * 13 * 13), np.uint8)
    cost, count, cls = np.zeros((1, 16), np.uint32), np.zeros((1, 16), np.uint64), np.zeros(1, np.int32)
    u32 = lambda c: np.array(c, np.uint32).ctypes.data_as(_u32p)
    call = lambda code, L, costs, w, n=1: lib.qecmc_class_minplus_chains(code, L, n, L_.u8(big), u32(costs), w, L_.u8(out), cost.ctypes.data_as(_u32p),
                                                                         count.ctypes.data_as(_u64p), L_.i32(cls))
    for code, L, costs, w, want, frags in M.REFUSED:
        assert call(code, L, costs, w) == want
        err = lib.qecmc_last_error()
        assert err.startswith(b"qecmc_class_minplus_chains:") and all(f in err for f in frags), err
    assert lib.qecmc_class_minplus_chains(ROTATED, 3, 1, None, u32(UNIT), 0, L_.u8(out), None, None, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert lib.qecmc_class_minplus_chains(ROTATED, 3, 1, L_.u8(big), None, 0, L_.u8(out), None, None, None) == -1
    assert lib.qecmc_class_minplus_chains(ROTATED, 3, 1, L_.u8(big), u32(UNIT), 0, None, None, None, None) == -1
    # a valid call gets as far as the device lookup: no device, no CPU fallback
    have = L_.device_count() >= 1
    for n in (1, 0):
        assert call(ROTATED, 3, UNIT, 0, n) == (0 if have else -2)
    if not have:
        assert b"no CPU fallback" in lib.qecmc_last_error()
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.shortest_chains("rotated", np.zeros((1, 3, 3), np.uint8))


def test_harness_refuses_the_option_under_another_method():
    from qecmc import harness
    for method in ("PTEQ", "exact", "STDC"):
        with pytest.raises(ValueError, match="params\\['correction'\\]='shortest' is built for method min_weight, not " + method):
            harness.generate(dict(code="rotated", size=5, p_error=0.1, method=method, correction="shortest"), 4, corrections=method != "STDC")
    with pytest.raises(ValueError, match="params\\['correction'\\]='shortest' is built for method min_weight, not exact"):
        harness.decode_syndromes(dict(code="rotated", size=3, p_error=0.1, method="exact", correction="shortest"), np.zeros((1, 16), np.uint8), corrections=True)
    with pytest.raises(ValueError, match="params\\['correction'\\]='greedy'"):
        harness.generate(dict(code="rotated", size=5, p_error=0.1, method="min_weight", correction="greedy"), 4, corrections=True)


# ------------------------------------------------------------------------------------------------------ the Python layer
class _TwinLibrary:
    """the library with qecmc_class_minplus_chains answered by the host twin: what the Python layer does around the call needs no device"""

    def __init__(self, real, T):
        self._real, self._T = real, T

    def __getattr__(self, name):
        return getattr(self._real, name)

    def qecmc_class_minplus_chains(self, *args):
        return self._T.qt_class_minplus_chains(*args, None, 0)


def test_python_layer_shapes_unique_and_min_weight_corrections(T, monkeypatch):
    import qecmc
    assert qecmc.shortest_chains is ex.shortest_chains and qecmc.min_weight_corrections is ex.min_weight_corrections
    real = L_.lib()
    monkeypatch.setattr(ex.L_, "lib", lambda: _TwinLibrary(real, T))
    for code, L, lds_width in [(ROTATED, 5, 0), (TORIC, 3, 6), (PLANAR, 3, 0)]:
        chains = random_errors(code, L, 5, np.random.default_rng([78, code, L]))
        r = ex.shortest_chains(NAME[code], chains, MIXED, lds_width=lds_width)
        out, cost, count, cls = twin(T, code, L, chains, MIXED, lds_width)
        ncls = 16 if code == TORIC else 4
        assert r["chains"].shape == (5, ncls) + state_shape(code, L) and r["chains"].dtype == np.uint8
        assert np.array_equal(r["chains"].reshape(out.shape), out)
        assert np.array_equal(r["cost"], cost) and np.array_equal(r["count"], count) and np.array_equal(r["cls"], cls)
        assert r["unique"].dtype == bool and np.array_equal(r["unique"], count == 1) and np.array_equal(r["saturated"], count == 0)
        inf = SC.info(T, code, L, lds_width)[1]
        assert (r["width"], r["held"]) == (inf["width"], inf["held"])
        flat = ex.shortest_chains(code, chains.reshape(5, -1), MIXED, size=L, lds_width=lds_width)
        assert np.array_equal(flat["chains"], r["chains"])
        m = ex.min_weight_corrections(NAME[code], chains, MIXED, lds_width=lds_width)
        target = ex._rank_classes(cost, count)
        assert np.array_equal(m["target"], target) and m["correction"].shape == chains.shape
        assert np.array_equal(m["correction"], r["chains"][np.arange(5), target])
        assert np.array_equal(m["weight"], cost.min(axis=1)) and m["weight"].dtype == np.uint32
    for bad in [(0, 1, 1), (0, 1.5, 1, 1), (0, -1, 1, 1)]:
        with pytest.raises(ValueError, match="integer costs"):
            ex.shortest_chains("rotated", np.zeros((2, 3, 3), np.uint8), bad)
    monkeypatch.undo()                                                          # (the library itself refuses on the host, and keeps the message)
    with pytest.raises(L_.QecmcError, match="qecmc_class_minplus_chains: cost\\[3\\]=256"):
        qecmc.shortest_chains("rotated", np.zeros((2, 3, 3), np.uint8), (0, 1, 1, 256))


# ------------------------------------------------------------------------------------------------------ the sanitizers
def test_minplus_trace_under_sanitizers():
    """a stand-alone program (its own main) built from class_minplus_trace.hpp with -fsanitize=address,undefined: the trace plans against the cut plans,
    the twin over poisoned scratch, decision words and outputs allocated at their exact size; run as a child process"""
    run_selftest("minplus_trace_asan", "class_minplus_trace_selftest_asan")
