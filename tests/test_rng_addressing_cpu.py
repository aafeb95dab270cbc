"""Philox addressing beyond 32 bits, the reference's half (no GPU): what must hold of the oracle alone for tests/test_gpu_rng_addressing.py to prove
something.  For every row of the edge table (tests/rng_edges.py) the run across it starts at least three ladder steps below the boundary and ends above it
-- by arithmetic on the run's first and last index --, and the oracle's result at the edge address differs from its result at each truncated address: the
seed with its high word cleared, first_syndrome = 0, step 0 (single chains: k0 - 2^32).  So a kernel that dropped seed_hi, kept a block index in 32 bits or
let k[47:32] bleed into `sub` cannot agree with the oracle there.  The shapes and registry rows the GPU file runs are checked here too: the kernel each one
is meant for is the one the host chooser picks, and the oracle's half of it is not vacuous with the 64-bit seeds.  The host-side refusal of indices past
the 48-bit counter (rng_range_check(), csrc/plan_host.hpp) is exercised through the host test API."""
import ctypes as C

import numpy as np
import pytest

import kernel_cases as K
import rng_edges as E

# the ladders compared on the oracle alone: both ends of the first wavefront, the second one's first and last live lane, and four in between
LADDERS = (0, 1, 20, 33, 47, 63, 64, 69)
INVALID = -1


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def T():
    lib = K.tables_lib()
    lib.qt_rng_range_check.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int]
    return lib


def _differing(a, b):
    """the ladders whose final rung states differ"""
    return int((a["states"].reshape(len(a["states"]), -1) != b["states"].reshape(len(b["states"]), -1)).any(axis=1).sum())


def test_the_table_names_every_stream_and_claims_no_more():
    assert len({e["id"] for e in E.EDGES}) == len(E.EDGES) == 8
    for e in E.EDGES:
        assert "philox.hpp" in e["stream"] or "DESIGN.md" in e["stream"], e["id"]
    assert any("refinement" in s for s in E.NOT_SHOWN) and any("criterion" in s for s in E.NOT_SHOWN)
    used = {e for s in E.SHAPES for e in s["edges"]}
    assert used == set(E.EDGE), set(E.EDGE) - used                      # every edge is run by some shape on the GPU
    for s in E.SHAPES:
        assert s["site"].split(":")[0].split(",")[0] in ("ladder_kernel.hpp", "ladder_wu.hpp"), s["id"]
        for e in s["edges"]:
            assert ("random", "sweep", "colour", "wave").index(s["scan"]) in E.EDGE[e]["scans"], (s["id"], e)
            assert E.iters_of(e, s["iters"]) == s["iters"], (s["id"], e)
    sites = " ".join(s["site"] for s in E.SHAPES)
    for form in ("b0 + bi", "kb - (kq >> 2)", "(kb1 >> 1) + jj", "k >> 7", "T * nch + c", "wi * 64 + lane", "kb - (kq >> 1)"):
        assert form in sites, form


# (at iters = 10 the runs start near these steps: the figures the table was designed against)
NEAR = {"proposal 2^32": 429496727, "proposal 2^33": 858993456, "proposal 2^34": 1717986915, "proposal 2^39": 54975581385, "step 2^32": 4294967293,
        "wave acceptance, nch = 3": 1431655763, "wave pick window": 805306365, "top of the counter": 28147497671058}


@pytest.mark.parametrize("iters", [1, 7, 10, 25])
@pytest.mark.parametrize("edge", [e["id"] for e in E.EDGES])
def test_the_run_crosses_the_edge(edge, iters):
    iters = E.iters_of(edge, iters)
    first, last = E.check_crossing(edge, iters)
    s0 = E.step0(edge, iters)
    assert 0 < s0 and (s0 + E.STEPS) * iters <= E.LIMIT - E.SLACK
    if iters == E.iters_of(edge, 10):
        assert abs(s0 - NEAR[edge]) <= 5, (edge, s0)
    print(edge, "iters", iters, "step0", s0, "indices", first, "..", last)


def _toric(scan, iters):
    return dict(code="toric", L=5, Nc=4, iters=iters, p=0.15, scan=("random", "sweep", "colour", "wave")[scan])


@pytest.mark.parametrize("edge,scan", [(e["id"], scan) for e in E.EDGES for scan in e["scans"]])
def test_truncating_the_address_changes_the_reference(orc, edge, scan):
    """toric L = 5, Nc = 4, p = 0.15, six steps, eight ladders: at least three quarters of them end in other rung states at each truncated address"""
    iters = E.iters_of(edge)
    shape, s0 = _toric(scan, iters), E.step0(edge, iters)
    init = E.make_init("toric", 5, E.N, 5)
    at = E.oracle_run(orc, shape, init, E.SEED, E.FIRST, s0, ladders=LADDERS)
    for what, (seed, first, step) in {"seed_hi cleared": (E.SEED & 0xFFFFFFFF, E.FIRST, s0), "first_syndrome = 0": (E.SEED, 0, s0),
                                      "step 0": (E.SEED, E.FIRST, 0), "step0 mod 2^32": (E.SEED, E.FIRST, s0 & 0xFFFFFFFF)}.items():
        if (seed, first, step) == (E.SEED, E.FIRST, s0):
            continue                                                       # (an edge whose run starts below 2^32 steps: nothing to cut off)
        n = _differing(at, E.oracle_run(orc, shape, init, seed, first, step, ladders=LADDERS))
        print(edge, "scan", scan, what, n, "of", len(LADDERS), "ladders differ")
        assert 4 * n >= 3 * len(LADDERS), (what, n)


@pytest.mark.parametrize("name", list(E.SEEDS))
def test_every_seed_needs_its_high_word(orc, name):
    seed, s0 = E.SEEDS[name], E.step0("proposal 2^33", 10)
    init = E.make_init("toric", 5, E.N, 5)
    for scan in (0, 3):
        at = E.oracle_run(orc, _toric(scan, 10), init, seed, E.FIRST, s0, ladders=LADDERS)
        n = _differing(at, E.oracle_run(orc, _toric(scan, 10), init, seed & 0xFFFFFFFF, E.FIRST, s0, ladders=LADDERS))
        assert 4 * n >= 3 * len(LADDERS), (name, scan, n)
        n = _differing(at, E.oracle_run(orc, _toric(scan, 10), init, seed >> 32 << 32 if seed & 0xFFFFFFFF else seed ^ 1, E.FIRST, s0, ladders=LADDERS))
        assert 4 * n >= 3 * len(LADDERS), (name, scan, n, "low word")


@pytest.mark.parametrize("shape", [s["id"] for s in E.SHAPES])
def test_the_shapes_run_the_kernels_they_are_there_for(orc, T, shape):
    """the host chooser's kernel for the launch is the one the table names, and on the shape's own inputs the oracle tells the edge address from the
    truncated ones (the ladders of both wavefronts)"""
    s = E.SHAPE[shape]
    assert K.predict(T, E.shape_case(s)) == s["kernel"]
    init = E.make_init(s["code"], s["L"], E.N, 5)
    pick = (0, 33, 63, 69)
    for edge in s["edges"]:
        s0 = E.step0(edge, s["iters"])
        E.check_crossing(edge, s["iters"])
        at = E.oracle_run(orc, s, init, E.SEED, E.FIRST, s0, ladders=pick)
        for seed, first, step in ((E.SEED & 0xFFFFFFFF, E.FIRST, s0), (E.SEED, 0, s0), (E.SEED, E.FIRST, 0)):
            n = _differing(at, E.oracle_run(orc, s, init, seed, first, step, ladders=pick))
            assert 4 * n >= 3 * len(pick), (shape, edge, seed, first, step, n)


@pytest.mark.parametrize("aligned", [True, False], ids=["k0 % 4 == 0", "k0 % 4 != 0"])
@pytest.mark.parametrize("boundary", E.CHAIN_BOUNDARIES, ids=["2^32", "2^33", "2^34"])
@pytest.mark.parametrize("chain", [c["id"] for c in E.CHAINS])
def test_a_single_chain_does_not_alias(orc, chain, boundary, aligned):
    """CHAIN_ITERS proposals from k0 across the boundary: the run at k0 - 2^32 ends elsewhere, and so does the part of the run past the boundary when its
    indices lose 2^32 (with a handful of proposals both runs can reject everything and compare equal: hence a few hundred, on hot chains -- rng_edges.CHAINS)"""
    k0, m = E.k0_of(boundary, aligned), E.chain_init(chain)
    assert k0 < boundary < k0 + E.CHAIN_ITERS and k0 + E.CHAIN_ITERS + E.SLACK < E.LIMIT
    for pl in E.CHAIN[chain]["p_logical"]:
        at = E.oracle_chain(orc, chain, m, pl, E.CHAIN_ITERS, E.SEED, k0)
        assert not np.array_equal(at, m)
        if k0 >= 1 << 32:
            assert not np.array_equal(at, E.oracle_chain(orc, chain, m, pl, E.CHAIN_ITERS, E.SEED, k0 - (1 << 32))), (chain, pl, "k0 - 2^32")
        head = E.oracle_chain(orc, chain, m, pl, boundary - k0, E.SEED, k0)
        tail = E.CHAIN_ITERS - (boundary - k0)
        assert not np.array_equal(E.oracle_chain(orc, chain, head, pl, tail, E.SEED, boundary), E.oracle_chain(orc, chain, head, pl, tail, E.SEED, boundary - (1 << 32))), \
            (chain, pl, "past the boundary")
        assert not np.array_equal(at, E.oracle_chain(orc, chain, m, pl, E.CHAIN_ITERS, E.SEED & 0xFFFFFFFF, k0)), (chain, pl, "seed_hi")
        assert not np.array_equal(at, E.oracle_chain(orc, chain, m, pl, E.CHAIN_ITERS, E.SEED, k0, stream=E.CHAIN_STREAM & 0xFFFF)), (chain, pl, "syndrome index")


@pytest.fixture(scope="module")
def whole_runs():
    return E.whole_run_cases(K.load_cases())


def test_the_whole_run_selection_covers_the_entry_points(whole_runs):
    what = " | ".join(w for _, w in E.WHOLE_RUN)
    for need in ("fixed length", "criterion, depolarizing", "work queue", "scan = wave on its queue", "scan = colour", "return_swap_stats", "pteq_shortest_batch",
                 "ptdc_batch", "biased", "alpha"):
        assert need in what, need
    assert {c["seed"] for c in whole_runs} == set(E.SEEDS.values())
    assert {c["entry"] for c in whole_runs} == set(K.ENTRIES)


@pytest.mark.parametrize("i", range(len(E.WHOLE_RUN)), ids=[l for l, _ in E.WHOLE_RUN])
def test_the_whole_run_rows_stay_meaningful_with_the_new_seed(T, whole_runs, i):
    """vacuous() depends on the seed: a row that turns vacuous is replaced in rng_edges.WHOLE_RUN, not excused.  And the oracle's answer needs the seed's
    high word and the syndrome index's high bits."""
    c = whole_runs[i]
    assert K.predict(T, c) == c["label"]
    init = K.make_init(c)
    ref = K.run_oracle(c, init)
    assert K.vacuous(c, init, ref) == []
    keys = ("hist", "mhist") if c["entry"] == "ptdc" else ("counts", "tops0", "steps_done", "states")
    for cut in (dict(seed=c["seed"] & 0xFFFFFFFF), dict(first_syndrome=c["first_syndrome"] & 0xFFFF)):
        if cut.get("seed") == c["seed"]:
            continue
        other = K.run_oracle(dict(c, **cut), init)
        assert any(k in ref and not np.array_equal(ref[k], other[k]) for k in keys), cut


# ---------------------------------------------------------------------------------------------------------------- the refusal, on the host
def _check(T, resume, step0, nsteps, prop0, iters):
    msg = C.create_string_buffer(600)
    return T.qt_rng_range_check(int(resume), step0, nsteps, prop0, iters, msg, len(msg)), msg.value.decode()


@pytest.mark.parametrize("iters", [1, 10, 25])
def test_the_last_index_plus_64_stays_below_2_48(T, iters):
    steps = E.STEPS
    last_ok = (E.LIMIT - E.SLACK) // iters - steps                       # = step0("top of the counter")
    assert last_ok == E.step0("top of the counter", iters)
    for resume in (1, 0):
        assert _check(T, resume, last_ok, steps, last_ok * iters, iters) == (0, "")
        rc, msg = _check(T, resume, last_ok + 1, steps, (last_ok + 1) * iters, iters)
        assert rc == INVALID and str((last_ok + 1) * iters) in msg and str(1 << 48) in msg and "64" in msg, msg
    # a single chain: k0 + iters <= 2^48 - 64
    k0 = E.LIMIT - E.SLACK - iters
    assert _check(T, 0, 0, 1, k0, iters)[0] == 0
    rc, msg = _check(T, 0, 0, 1, k0 + 1, iters)
    assert rc == INVALID and str(k0 + 1) in msg


def test_products_that_overflow_64_bits_are_refused(T):
    big = 1 << 63
    for args in ((1, big, 6, 0, 2), (1, (1 << 64) - 1, 1, 0, 10), (0, 0, big, 0, 2), (0, 0, 1, (1 << 64) - 5, 10), (0, big, big, 0, 0)):
        rc, msg = _check(T, *args)
        assert rc == INVALID and msg, args
    rc, msg = _check(T, 1, big, 6, 0, 2)
    assert "overflow" in msg and str(big) in msg
    # the ladder-step index on its own (the swap stream's block index)
    assert _check(T, 0, E.LIMIT - E.SLACK - 6, 6, 0, 1)[0] == 0
    rc, msg = _check(T, 0, E.LIMIT - E.SLACK - 5, 6, 0, 1)
    assert rc == INVALID and "swap" in msg
    # well inside: accepted
    assert _check(T, 1, 0, 1 << 20, 0, 10) == (0, "") and _check(T, 0, 1 << 40, 100, 1 << 44, 10) == (0, "")
