"""The exact chain sampler on the tiled plans (csrc/class_sample_tiled.hpp), without a GPU: the twin sample_tiled_host, compiled by g++ into the
host-table test library (qt_class_sample_tiled, qt_class_sample_tiled_plan, qt_class_sample_tiled_pass), and the Python layer around it.

What is pinned: the plan -- pair_off and forget_tile follow the segment table, bytes_per_job is 128 times the traceback's bytes per pair wherever
tile_width >= 7, the jobs of a pass obey the cap --; the twin against sample_host byte for byte (chains, classes, z as bits) in both modes wherever
the two plans have one stream, which carries the chi-square pins of tests/test_class_sample_cpu.py over to this twin; at rotated L = 13 and planar
L = 8, the first shapes only this route takes, every sample has the input's syndrome and its class by the oracle and z is sweep_tiled_host's bits; THE
LAW at rotated L = 13: the mean error count of 4 096 draws per class against d log Z_c / d log t, a central difference of sweep_tiled_host that
does not touch the sampler, within 5 of the draws' own standard errors (the project's bound); the low-p limit against the (min, +)
family on the tiled plans; a sample as a function of its address; forced holds; site tables, erasures; every refusal by name, the record cap with
its bytes; the 2^-960 floor; the Python layer; the ABI version and N == 0.  (The sanitizers: tests/test_class_sample_tiled_resources.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

import test_class_minplus_tiled_cpu as MT
import test_class_minplus_tiled_trace_cpu as TT
import test_class_sample_cpu as SA
import test_class_sweep_site_cpu as SS
import test_class_sweep_tiled_cpu as ST
from qecmc import _lib as L_
from qecmc import exact as ex
from qecmc import harness
from test_corrections_cpu import classes, generators, syndromes
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, state_shape
from util_minplus_trace import qubit_cells

NAME = MT.NAME
SEED = 20261021
CAP, CAP_MAX = 4 << 30, 64 << 30
INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -4                                    # QECMC_ERR_* (include/qecmc.h)
_u8p, _u32p, _i32p, _u64p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
PREFIX, SITE_PREFIX = "qecmc_class_sample_tiled: ", "qecmc_class_sample_tiled_site: "
DEPOL, BIASED, FLAT = SA.DEPOL, SA.BIASED, SA.FLAT
nq_of = MT.nq_of


def load_twin():
    """the host-table test library with the tiled sampler's entry points next to every sibling's (tests/test_gpu_class_sample_tiled.py compares the GPU
    with it)"""
    lib = SA.load_twin()
    TT.load_twin()                                                              # (one CDLL per path: the siblings' argtypes on the same object)
    lib.qt_class_sample_tiled.restype = lib.qt_class_sample_tiled_plan.restype = C.c_int
    lib.qt_class_sample_tiled.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _f64p, _f64p, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                          C.c_int, _u8p, _i32p, _f64p, C.c_char_p, C.c_int]
    lib.qt_class_sample_tiled_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, _i32p, _u32p, _u32p, _u64p, _u32p, C.c_int, _u64p, C.c_char_p, C.c_int]
    lib.qt_class_sample_tiled_pass.restype = C.c_uint32
    lib.qt_class_sample_tiled_pass.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def twin_rc(T, code, L, chains, w=None, wq=None, K=1, seed=SEED, first=0, mode=0, hbm_width=0, tile_width=0, record_bytes=0):
    """(rc, message, chains uint8[N, ncls, K, nq] or [N, K, nq], cls int32[N, K], z float64[N, ncls]) of the host twin; the outputs start out poisoned.
    wq: float[rows, nq, 4] or [nq, 4]"""
    flat = np.ascontiguousarray(chains, dtype=np.uint8)
    nq = flat.shape[-1] if flat.ndim == 2 else nq_of(code, L)                   # (rows given flat are taken as they are: a refused (code, L) reads none)
    flat = flat.reshape(-1, nq)
    n, ncls = len(flat), 16 if code == TORIC else 4
    kk = K if 0 < K < 1 << 20 else 1
    out = np.full((n, kk, nq) if mode == 1 else (n, ncls, kk, nq), 0xEE, np.uint8)
    cls, z = np.full((n, kk), 99, np.int32), np.full((n, ncls), -1.0)
    msg = C.create_string_buffer(640)
    wp = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    tab = None if wq is None else np.ascontiguousarray(wq, dtype=np.float64).reshape(-1, nq, 4)
    rc = T.qt_class_sample_tiled(code, L, n, flat.ctypes.data_as(_u8p), None if wp is None else wp.ctypes.data_as(_f64p), None if tab is None else tab.ctypes.data_as(_f64p),
                                 0 if tab is None else len(tab), hbm_width, tile_width, record_bytes, K, seed, first, mode, out.ctypes.data_as(_u8p), cls.ctypes.data_as(_i32p),
                                 z.ctypes.data_as(_f64p), msg, 640)
    return rc, msg.value.decode(), out, cls, z


def twin(T, code, L, chains, **kw):
    rc, msg, out, cls, z = twin_rc(T, code, L, chains, **kw)
    assert rc == 0, msg
    return out, cls, z


def sample_plan(T, code, L, hbm_width=0, tile_width=0, cap=0):
    """dict(forget_gen int32[n], forget_chains uint8[n, nq], forget_tile uint32[n, 4], pair_off uint64[n + 1], seg_forget uint32[segments], n_forget,
    job_bytes, W, cap, cap_max, state_bits, segments, held), or (message, the numbers written before the refusal) where the plan is refused"""
    _, inf, _ = ST.info(T, code, L, hbm_width, tile_width)
    W, rows = (inf["nq"] + 15) // 16, max(inf["n_gen"], inf["segments"], 1)
    gen, words, tile, seg = np.full(rows, -1, np.int32), np.zeros(rows * W, np.uint32), np.zeros(rows * 4, np.uint32), np.zeros(rows, np.uint32)
    off, out8, msg = np.zeros(rows + 1, np.uint64), np.zeros(8, np.uint64), C.create_string_buffer(640)
    n = T.qt_class_sample_tiled_plan(code, L, hbm_width, tile_width, cap, gen.ctypes.data_as(_i32p), words.ctypes.data_as(_u32p), tile.ctypes.data_as(_u32p),
                                     off.ctypes.data_as(_u64p), seg.ctypes.data_as(_u32p), rows, out8.ctypes.data_as(_u64p), msg, 640)
    d = dict(zip(("n_forget", "job_bytes", "W", "cap", "cap_max", "state_bits", "segments", "held"), (int(x) for x in out8)))
    if n < 0:
        return msg.value.decode(), d
    words, q = words[:n * W].reshape(n, W), np.arange(inf["nq"])
    d.update(forget_gen=gen[:n], forget_chains=((words[:, q >> 4] >> ((q & 15) * 2).astype(np.uint32)) & 3).astype(np.uint8), forget_tile=tile[:4 * n].reshape(n, 4),
             pair_off=off[:n + 1], seg_forget=seg[:d["segments"]])
    return d


def check_samples(code, L, chains, out, cls=None):
    """every sample: the input's syndrome and its class, by the oracle.  out [N, ncls, K, nq] (cls None) or [N, K, nq] with cls [N, K]"""
    assert out.max() <= 3
    syn = syndromes(code, np.asarray(chains).reshape((-1,) + state_shape(code, L)))
    for s in range(len(out)):
        got = out[s].reshape((-1,) + state_shape(code, L))
        assert np.array_equal(syndromes(code, got), np.broadcast_to(syn[s], (len(got),) + syn[s].shape)), s
        want = np.repeat(np.arange(out.shape[1]), out.shape[2]) if cls is None else cls[s]
        assert np.array_equal(classes(code, got), want), s


# ------------------------------------------------------------------------------------------------------ the plan
# every (code, L, hbm_width, tile_width) the tests of this file and of the GPU file run, and the shapes DESIGN.md 4.1v names
PLANS = [(XZZX, 5, 0, 0), (XZZX, 5, 0, 4), (ROTATED, 7, 0, 0), (ROTATED, 7, 0, 5), (ROTATED, 7, 0, 7), (ROTATED, 9, 0, 0), (ROTATED, 9, 0, 8), (PLANAR, 5, 0, 0),
         (TORIC, 3, 13, 0), (TORIC, 3, 0, 6), (TORIC, 3, 8, 4), (TORIC, 5, 13, 0), (ROTATED, 13, 0, 0), (ROTATED, 13, 0, 8), (ROTATED, 13, 0, 13), (ROTATED, 15, 0, 0),
         (PLANAR, 8, 0, 0), (ROTATED, 17, 0, 0), (ROTATED, 21, 0, 0), (XZZX, 21, 0, 0), (PLANAR, 12, 0, 0), (TORIC, 7, 0, 0)]


@pytest.mark.parametrize("code,L,hbm_width,tile_width", PLANS)
def test_plan_names_every_forgets_generator_and_its_place_in_the_record(T, code, L, hbm_width, tile_width):
    gens = generators(code, L)
    _, inf, _ = ST.info(T, code, L, hbm_width, tile_width)
    sp = sample_plan(T, code, L, hbm_width, tile_width, cap=CAP_MAX)
    tw = tile_width or 11
    print("%s L=%d hbm %d tile %d: width %d, held %d, %d FORGETs, %d bytes per job" % (NAME[code], L, hbm_width, tile_width, inf["width"], inf["held"], sp["n_forget"],
                                                                                      sp["job_bytes"]))
    assert sp["cap"] == CAP and sp["cap_max"] == CAP_MAX and sp["W"] == (inf["nq"] + 15) // 16
    assert (sp["state_bits"], sp["segments"], sp["held"]) == (max(inf["width"], tw), inf["segments"], inf["held"])
    assert np.array_equal(sp["forget_chains"], gens[sp["forget_gen"]])           # forget_words[i] is generator forget_gen[i] of the oracle's table
    held = ST.held_of(T, code, L, hbm_width, tile_width)[0].tolist()
    assert sorted(held + sp["forget_gen"].tolist()) == list(range(len(gens)))   # held and retired: the table, each exactly once
    # forget_tile and pair_off, from the segment table and the wide stream alone
    ops, off, fi, half = ST.ops_of(T, code, L, hbm_width, tile_width), 0, 0, 1 << (tw - 1)
    for s, sg in enumerate(ST.segments_of(T, code, L, hbm_width, tile_width)):
        assert sp["seg_forget"][s] == fi
        for kind, slot, top, mask, pairs, qubit in ops[sg["op_first"]:sg["op_first"] + sg["op_count"]]:
            if kind != ST.FORGET:
                continue
            local = bin(sg["tile"] & ((1 << slot) - 1)).count("1")
            assert sp["forget_tile"][fi].tolist() == [sg["tile"], sg["live"] & ~sg["tile"], local, off] and int(sp["pair_off"][fi]) == off, (s, fi)
            assert sg["tile"] >> slot & 1 and sg["n_tiles"] == 1 << bin(sg["live"] & ~sg["tile"]).count("1")
            off += sg["n_tiles"] * half
            fi += 1
    assert fi == sp["n_forget"] and int(sp["pair_off"][fi]) == off and sp["job_bytes"] == 16 * off <= CAP_MAX
    tr = TT.trace_plan(T, code, L, hbm_width, tile_width)
    assert tr["n_forget"] == sp["n_forget"] and np.array_equal(tr["forget_gen"], sp["forget_gen"])          # the FORGETs are the traceback's
    if tw >= 7:
        assert sp["job_bytes"] == 128 * tr["pair_bytes"]                        # a 16-byte pair for every decision bit


def test_bytes_per_job_of_the_shapes_design_names(T):
    got = {(c, L): sample_plan(T, c, L, cap=CAP_MAX)["job_bytes"] for c, L in ((ROTATED, 13), (ROTATED, 15), (ROTATED, 17), (ROTATED, 21), (PLANAR, 12), (TORIC, 7))}
    print(got)
    assert got[(ROTATED, 13)] == 128 * 496896 and got[(ROTATED, 17)] == 128 * 13082880 and got[(ROTATED, 21)] == 128 * 303650944
    assert got[(PLANAR, 12)] == 128 * 258412928 and got[(TORIC, 7)] == 128 * 77956992
    assert got[(ROTATED, 17)] <= CAP < got[(TORIC, 7)] < got[(PLANAR, 12)] < got[(ROTATED, 21)] <= CAP_MAX


def test_jobs_of_a_pass_obey_the_workspace_and_the_cap(T):
    P = T.qt_class_sample_tiled_pass
    for code, L, hbm_width, tile_width in PLANS:
        sp = sample_plan(T, code, L, hbm_width, tile_width, cap=CAP_MAX)
        units = ST.info(T, code, L, hbm_width, tile_width)[1]["pass_units"]
        for left in (1, 2, 7, 16, 2049, 1 << 20):
            for cap in (0, 1 << 20, 3 * sp["job_bytes"], 3 * sp["job_bytes"] + 1):
                n = P(sp["state_bits"], sp["job_bytes"], left, cap)
                assert n == max(1, min(units, (cap or CAP) // sp["job_bytes"], left)), (code, L, left, cap)
    b13 = 128 * 496896
    assert P(16, b13, 4096, 0) == CAP // b13 == 67 and P(16, b13, 8, 3 * b13) == 3 and P(16, b13, 2, 3 * b13) == 2
    s17 = sample_plan(T, ROTATED, 17)
    assert P(s17["state_bits"], s17["job_bytes"], 4, 0) == 2 and P(24, 1 << 40, 5, 0) == 1                 # rotated L = 17 under the default cap; never 0


def test_a_job_past_the_cap_is_refused_by_name_with_its_bytes(T):
    b13 = 128 * 496896
    msg, d = sample_plan(T, ROTATED, 13, cap=b13 - 1)
    assert msg.startswith(PREFIX) and "%d bytes" % b13 in msg and str(b13 - 1) in msg and d["job_bytes"] == b13
    assert isinstance(sample_plan(T, ROTATED, 13, cap=b13), dict)
    for code, L in ((ROTATED, 21), (XZZX, 21), (TORIC, 7), (PLANAR, 12)):        # the default cap answers up to rotated / xzzx L = 17
        msg, d = sample_plan(T, code, L)
        assert msg.startswith(PREFIX) and "%d bytes" % d["job_bytes"] in msg and str(CAP) in msg and d["job_bytes"] > CAP, msg
    assert isinstance(sample_plan(T, ROTATED, 17), dict)


# ------------------------------------------------------------------------------------------------------ the twin is sample_host where the plans coincide
SAME = [(XZZX, 5, 0, 0, 3), (ROTATED, 7, 0, 0, 3), (ROTATED, 9, 0, 0, 2), (PLANAR, 5, 0, 0, 3), (TORIC, 3, 13, 13, 2), (TORIC, 5, 13, 13, 1)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("code,L,hbm_width,lds_width,n", SAME)
def test_twin_is_sample_host_byte_for_byte(T, code, L, hbm_width, lds_width, n, mode):
    assert TT.same_stream(T, code, L, hbm_width, lds_width)                     # op for op, holds included
    chains = MT.chains_of(code, L, n, seed=3)
    K = 5 if code == TORIC and L == 5 else 9
    got = twin(T, code, L, chains, w=BIASED, K=K, first=7, mode=mode, hbm_width=hbm_width)
    want = SA.twin(T, code, L, chains, w=BIASED, K=K, seed=SEED, first=7, mode=mode, lds_width=lds_width)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if L <= 7:
        for tile_width in (4, 7):                                               # (the twin knows nothing of tiles)
            one = twin(T, code, L, chains[:1], w=BIASED, K=K, first=7, mode=mode, hbm_width=hbm_width, tile_width=tile_width)
            assert all(a.tobytes() == b[:1].tobytes() for a, b in zip(one, want))


# ------------------------------------------------------------------------------------------------------ the shapes only this route takes
_first = {}


def first_shapes_case(T, code, L):
    """two syndromes, their twin draws in both modes (K = 3) and sweep_tiled_host's z, computed once (the GPU file reads the rotated L = 13 rows)"""
    if (code, L) not in _first:
        chains = MT.chains_of(code, L, 2, seed=13)
        _first[(code, L)] = (chains, twin(T, code, L, chains, w=DEPOL, K=3), twin(T, code, L, chains, w=DEPOL, K=3, mode=1), ST.twin(T, code, L, chains, DEPOL)[0])
    return _first[(code, L)]


@pytest.mark.parametrize("code,L", [(ROTATED, 13), (PLANAR, 8)])
def test_first_shapes_samples_have_the_syndrome_and_the_class_and_z_is_the_sweeps(T, code, L):
    chains, (out, _, z), (post, cls, z1), z_sweep = first_shapes_case(T, code, L)
    assert z.tobytes() == z_sweep.tobytes() == z1.tobytes()
    check_samples(code, L, chains, out)
    check_samples(code, L, chains, post, cls)
    for s in range(2):
        assert all(np.array_equal(post[s, k], out[s, cls[s, k], k]) for k in range(3))        # posterior[s, k] == every_class[s, cls[s, k], k]
    assert len(np.unique(out.reshape(-1, out.shape[-1]), axis=0)) > 12          # independent draws, not one chain per class


# ------------------------------------------------------------------------------------------------------ the law
def test_the_law_at_rotated_L13_by_the_derivative_of_log_Z(T):
    """Under weights (1, t, t, t) a class weight is Z_c(t) = sum over its chains of t^(errors), so d log Z_c / d log t is the mean error count of the
    class exactly.  The derivative is a central difference of sweep_tiled_host at relative step 1e-4 -- its error is of relative order 1e-8 against
    standard errors of 1e-2 --; the draws' mean must lie within 5 of its own standard errors of it (DESIGN.md 4.1s's bound)."""
    code, L, K, p, h = ROTATED, 13, 4096, 0.1, 1e-4
    t = (p / 3) / (1 - p)
    chains = MT.chains_of(code, L, 2, seed=21)
    out, _, z = twin(T, code, L, chains, w=[1.0, t, t, t], K=K)
    lo, hi = t * (1 - h), t * (1 + h)
    z_lo, z_hi = ST.twin(T, code, L, chains, [1.0, lo, lo, lo])[0], ST.twin(T, code, L, chains, [1.0, hi, hi, hi])[0]
    want = (np.log(z_hi) - np.log(z_lo)) / (np.log(hi) - np.log(lo))
    worst = 0.0
    for s in range(2):
        for c in range(4):
            n_err = np.count_nonzero(out[s, c], axis=1)
            mean, se = n_err.mean(), n_err.std(ddof=1) / np.sqrt(K)
            worst = max(worst, abs(mean - want[s, c]) / se)
            print("syndrome %d class %d: mean error count %.4f +- %.4f, d log Z / d log t = %.4f (%.2f standard errors)" % (s, c, mean, se, want[s, c],
                                                                                                                        (mean - want[s, c]) / se))
            assert se > 0 and abs(mean - want[s, c]) <= 5.0 * se
    assert worst > 0.0


# ------------------------------------------------------------------------------------------------------ the low-p limit
@pytest.mark.parametrize("code,L,hbm_width,tile_width,n,k", [(ROTATED, 13, 0, 0, 6, 2), (TORIC, 3, 8, 4, 4, 2), (ROTATED, 7, 0, 5, 4, 2)])
def test_low_p_samples_are_the_shortest_chains(T, code, L, hbm_width, tile_width, n, k):
    m = MT.few_errors(code, L, n, k, seed=5)
    want, cost, count, _ = TT.twin(T, code, L, m, (0, 1, 1, 1), hbm_width, tile_width)
    assert np.array_equal(cost, MT.twin(T, code, L, m, (0, 1, 1, 1), hbm_width, tile_width)[0])              # minplus_tiled_host's
    out, _, _ = twin(T, code, L, m, w=ex.depolarizing_w4(1e-12), K=2, hbm_width=hbm_width, tile_width=tile_width)
    cells = qubit_cells(generators(code, L))
    assert (count == 1).sum() >= 2
    for s in range(n):
        for c in range(out.shape[1]):
            for kk in range(2):
                assert np.count_nonzero(out[s, c, kk][cells]) == cost[s, c]
                if count[s, c] == 1:
                    assert np.array_equal(out[s, c, kk], want[s, c])


# ------------------------------------------------------------------------------------------------------ the address
@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4)])
def test_a_sample_is_a_function_of_its_address(T, code, L, hbm_width, tile_width):
    m = MT.chains_of(code, L, 4, seed=3)
    kw = dict(w=DEPOL, hbm_width=hbm_width, tile_width=tile_width)
    full, _, _ = twin(T, code, L, m, K=6, first=10, **kw)
    assert np.array_equal(twin(T, code, L, m, K=3, first=10, **kw)[0], full[:, :, :3])                      # K
    assert np.array_equal(twin(T, code, L, m[2:3], K=6, first=12, **kw)[0], full[2:3])                      # N, first_syndrome moved along
    assert np.array_equal(twin(T, code, L, m[[3, 1]], K=6, first=13, **kw)[0][0], full[3])                  # the order of the rows
    post, cls, _ = twin(T, code, L, m, K=6, first=10, mode=1, **kw)
    for s in range(4):
        assert all(np.array_equal(post[s, k], full[s, cls[s, k], k]) for k in range(6))
    assert not np.array_equal(twin(T, code, L, m, K=6, first=10, seed=SEED + 1, **kw)[0], full)             # seed
    assert not np.array_equal(twin(T, code, L, m, K=6, first=11, **kw)[0], full)                            # s
    assert not np.array_equal(full[:, :, 0], full[:, :, 1])                                                 # k
    assert np.array_equal(twin(T, code, L, m, K=6, first=10, record_bytes=1 << 30, **kw)[0], full)          # the cap


def test_tile_width_does_not_change_a_byte_at_rotated_L13(T):
    chains, (out, _, z), (post, cls, _), _ = first_shapes_case(T, ROTATED, 13)
    for tile_width in (8, 11, 13):
        got = twin(T, ROTATED, 13, chains[:1], w=DEPOL, K=3, tile_width=tile_width)
        assert got[0].tobytes() == out[:1].tobytes() and got[2].tobytes() == z[:1].tobytes()


# ------------------------------------------------------------------------------------------------------ forced holds
def test_forced_holds_draw_from_the_law_of_the_plan_with_none(T):
    """toric L = 3 at hbm_width 8: a job per sample, every sample its own pick.  z is the free plan's up to the order of the sums; syndrome and class
    by the oracle; the error counts of 1 024 draws per class follow the brute force's law (the chi-square of tests/test_class_sample_cpu.py)."""
    import util_class_sample as U
    assert sample_plan(T, TORIC, 3, 8, 4)["held"] > 0 == sample_plan(T, TORIC, 3, 13, 0)["held"]
    m = MT.chains_of(TORIC, 3, 1, seed=11)
    K = 1024
    out, _, z = twin(T, TORIC, 3, m, w=FLAT, K=K, hbm_width=8, tile_width=4)
    assert z.tobytes() == ST.twin(T, TORIC, 3, m, FLAT, 8, 4)[0].tobytes()
    assert np.allclose(z, twin(T, TORIC, 3, m, w=FLAT, K=1, hbm_width=13)[2], rtol=1e-13, atol=0)
    check_samples(TORIC, 3, m, out)
    for c, (chains, prob, _) in enumerate(U.class_law(TORIC, 3, m[0], FLAT)):
        want = np.bincount(np.count_nonzero(chains, axis=1), weights=prob, minlength=19)
        SA.check_law(np.bincount(np.count_nonzero(out[0, c], axis=1), minlength=19), want, "toric hbm_width 8 class %d by error count" % c)
    post, cls, _ = twin(T, TORIC, 3, m, w=FLAT, K=8, mode=1, hbm_width=8, tile_width=4)
    assert all(np.array_equal(post[0, k], out[0, cls[0, k], k]) for k in range(8))


# ------------------------------------------------------------------------------------------------------ site tables
@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4), (ROTATED, 13, 0, 0)])
def test_constant_rows_are_the_uniform_entry_point(T, code, L, hbm_width, tile_width):
    m = MT.chains_of(code, L, 2, seed=21)
    nq = nq_of(code, L)
    for mode in (0, 1):
        kw = dict(K=3, mode=mode, hbm_width=hbm_width, tile_width=tile_width)
        a = twin(T, code, L, m, w=BIASED, **kw)
        b = twin(T, code, L, m, wq=np.broadcast_to(BIASED, (nq, 4)), **kw)
        c = twin(T, code, L, m, wq=np.broadcast_to(BIASED, (2, nq, 4)), **kw)
        for x, y, v in zip(a, b, c):
            assert x.tobytes() == y.tobytes() == v.tobytes()


def test_a_table_row_per_syndrome_is_addressed_by_s(T):
    code, L = ROTATED, 7
    m = MT.chains_of(code, L, 3, seed=4)
    tabs = np.random.default_rng(8).uniform(0.05, 1.0, size=(3, L * L, 4))
    both = twin(T, code, L, m, wq=tabs, K=4, tile_width=5)
    assert both[2].tobytes() == SS.twin(T, "tiled", code, L, m, tabs, (0, 5))[0].tobytes()                    # sweep_tiled_site_host's bits
    check_samples(code, L, m, both[0])
    for s in range(3):
        one = twin(T, code, L, m[s:s + 1], wq=tabs[s], K=4, first=s, tile_width=5)
        assert one[0].tobytes() == both[0][s:s + 1].tobytes() and one[2].tobytes() == both[2][s:s + 1].tobytes()
    cut = SA.twin(T, code, L, m, wq=tabs, K=4, seed=SEED)                       # (nothing held: the cut plan's stream)
    assert cut[0].tobytes() == both[0].tobytes() and cut[2].tobytes() == both[2].tobytes()


def test_site_twin_does_not_read_the_planar_codes_unused_cells(T):
    m = MT.chains_of(PLANAR, 5, 2, seed=10)
    cells = harness._qubit_cells(PLANAR, 5).ravel()
    tabs = np.random.default_rng(9).uniform(0.05, 1.0, size=(2, 50, 4))
    poisoned = tabs.copy()
    poisoned[:, ~cells] = np.nan
    got, want = twin(T, PLANAR, 5, m, wq=poisoned, K=3), twin(T, PLANAR, 5, m, wq=tabs, K=3)
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()


def test_pure_erasure_at_rotated_L13(T):
    """every weight off the erased set is (1, 0, 0, 0): no sample carries an error there, whatever the draws; z counts the chains on the erased set"""
    code, L, K = ROTATED, 13, 64
    rng = np.random.default_rng(2)
    erased = rng.random((L, L)) < 0.45
    err = np.zeros((1, L, L), np.uint8)
    err[0][erased] = rng.integers(0, 4, size=int(erased.sum()))               # an error on the erased set: its syndrome has chains there
    tab = ex.erasure_site_w4([1.0, 0.0, 0.0, 0.0], erased).reshape(L * L, 4)
    post, cls, z = twin(T, code, L, err, wq=tab, K=K, mode=1)
    assert z.tobytes() == SS.twin(T, "tiled", code, L, err, tab[None], (0, 0))[0].tobytes()
    assert (z[0] == np.round(z[0])).all() and z[0].sum() >= 1.0                  # counts of chains: exact in float64
    assert (post[0][:, ~erased.ravel()] == 0).all()
    check_samples(code, L, err, post, cls)
    assert (z[0][cls[0]] > 0).all()                                             # a class of weight 0 is never drawn


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(T):
    m = MT.chains_of(ROTATED, 7, 2, seed=1)
    for kw, frag in [(dict(K=0), "K=0"), (dict(K=1 << 32), "K=4294967296"), (dict(K=1, mode=2), "mode=2"), (dict(K=1, first=(1 << 32) - 1), "exceed 32 bits"),
                     (dict(K=1, tile_width=3), "tile_width=3"), (dict(K=1, tile_width=14), "tile_width=14"), (dict(K=1, hbm_width=25), "hbm_width=25"),
                     (dict(K=1, hbm_width=10), "hbm_width=10"), (dict(K=1, record_bytes=CAP_MAX + 1), "record_bytes=%d" % (CAP_MAX + 1))]:
        rc, msg, *_ = twin_rc(T, ROTATED, 7, m, w=DEPOL, **kw)
        assert rc == INVALID and msg.startswith(PREFIX) and frag in msg, msg
        rc, msg, *_ = twin_rc(T, ROTATED, 7, m, wq=np.ones((49, 4)), **kw)
        assert rc == INVALID and msg.startswith(SITE_PREFIX) and frag in msg, msg
    for bad, frag in ((np.inf, "w[1]=inf"), (-0.5, "w[1]=-0.5"), (np.nan, "w[1]=nan")):
        rc, msg, *_ = twin_rc(T, ROTATED, 7, m, w=[1.0, bad, 0.1, 0.1])
        assert rc == INVALID and msg.startswith(PREFIX) and frag in msg
    rc, msg, *_ = twin_rc(T, ROTATED, 7, m, w=[0.0, 0.0, 0.0, 0.0])
    assert rc == INVALID and msg.startswith(PREFIX) and "all zero" in msg
    # what qecmc_class_sweep_tiled refuses of (code, L, widths), with its codes and in its words
    for code, L, hbm_width, tile_width, rc_want, frags in MT.TILED_REFUSED:
        rc_sweep, _, sweep_msg = ST.info(T, code, L, hbm_width, tile_width)
        nq = nq_of(code, L) if code in (TORIC, XZZX, ROTATED, PLANAR) and 2 <= L <= 64 else 9
        rc, msg, *_ = twin_rc(T, code, L, np.zeros((1, nq), np.uint8), w=DEPOL, hbm_width=hbm_width, tile_width=tile_width)
        assert rc == rc_sweep == rc_want and msg == PREFIX + sweep_msg.decode(), msg
    # the record cap, with the bytes, before anything is swept
    rc, msg, *_ = twin_rc(T, ROTATED, 21, np.zeros((1, 441), np.uint8), w=DEPOL)
    assert rc == UNSUPPORTED and msg.startswith(PREFIX) and "%d bytes" % (128 * 303650944) in msg and str(CAP) in msg, msg
    rc, msg, *_ = twin_rc(T, TORIC, 7, np.zeros((1, 98), np.uint8), wq=np.ones((98, 4)))
    assert rc == UNSUPPORTED and msg.startswith(SITE_PREFIX) and "%d bytes" % (128 * 77956992) in msg, msg
    rc, msg, *_ = twin_rc(T, ROTATED, 13, np.zeros((1, 169), np.uint8), w=DEPOL, record_bytes=1 << 20)
    assert rc == UNSUPPORTED and "%d bytes" % (128 * 496896) in msg and str(1 << 20) in msg
    # the site table
    tab = np.ones((49, 4))
    tab[4] = 0.0
    rc, msg, *_ = twin_rc(T, ROTATED, 7, m, wq=tab)
    assert rc == INVALID and msg.startswith(SITE_PREFIX) and "qubit 4" in msg
    rc, msg, *_ = twin_rc(T, ROTATED, 7, MT.chains_of(ROTATED, 7, 3), wq=np.ones((2, 49, 4)))
    assert rc == INVALID and msg.startswith(SITE_PREFIX + "wq_rows=2")
    # a zero class in mode 0 names the row and the class; mode 1 draws from the classes that are left
    zero = np.zeros((2, 7, 7), np.uint8)
    zero[1, 0, 0] = 1
    only_identity = [1.0, 0.0, 0.0, 0.0]
    rc, msg, _, _, z = twin_rc(T, ROTATED, 7, zero, w=only_identity, tile_width=5)
    assert rc == INVALID and msg.startswith(PREFIX + "row 0, class 1:") and z[0, 0] == 1.0
    rc, msg, out, cls, z = twin_rc(T, ROTATED, 7, zero[:1], w=only_identity, K=3, mode=1, tile_width=5)
    assert rc == 0 and (cls == 0).all() and (out == 0).all()
    rc, msg, *_ = twin_rc(T, ROTATED, 7, zero, w=only_identity, K=3, mode=1, tile_width=5)
    assert rc == INVALID and msg.startswith(PREFIX + "row 1: the class weights total 0")


def test_the_floor_of_the_law_in_check_sample_zs_words(T):
    """a class weight (mode 0) or a row total (mode 1) below 2^-960 is refused by row and class, in the words of the cut route"""
    code, L = ROTATED, 7
    m = MT.chains_of(code, L, 1, seed=2)
    z1 = twin(T, code, L, m, w=FLAT, K=1, tile_width=5)[2]
    scale = float((2.0 ** -975 / z1.max()) ** (1.0 / 49))                       # every chain carries 49 factors: z scales with scale^49
    w = FLAT * scale
    rc, msg, _, _, z = twin_rc(T, code, L, m, w=w, tile_width=5)
    assert rc == INVALID and 0 < z[0].max() < 2.0 ** -961
    assert re.match(r"qecmc_class_sample_tiled: row 0, class 0: the class weight is \S+, below 2\^-960 = \S+ it underflows into the subnormal range", msg), msg
    rc_cut, msg_cut, *_ = SA.twin_rc(T, code, L, m, w=w)
    assert rc_cut == rc and msg_cut == msg.replace("qecmc_class_sample_tiled:", "qecmc_class_sample:")         # the same words
    rc, msg, *_ = twin_rc(T, code, L, m, w=w, mode=1, tile_width=5)
    assert rc == INVALID and re.match(r"qecmc_class_sample_tiled: row 0: the class weights total \S+, below 2\^-960", msg), msg
    ok = FLAT * float((2.0 ** -940 / z1.min()) ** (1.0 / 49))                   # above the floor: drawn, and every chain has weight > 0
    out, _, z = twin(T, code, L, m, w=ok, K=2, tile_width=5)
    assert z.min() >= 2.0 ** -961
    check_samples(code, L, m, out)


def test_the_library_refuses_on_the_host_and_n_0_and_the_abi(T):
    lib = L_.lib()
    assert lib.qecmc_abi_version() == 4
    chains, w = np.zeros((1, 441), np.uint8), np.ascontiguousarray(DEPOL)
    out, cls, z = np.zeros((1, 4, 1, 441), np.uint8), np.zeros((1, 1), np.int32), np.zeros((1, 4))

    def call(code, L, n, weights, hbm_width=0, tile_width=0, record_bytes=0, K=1, mode=0, chain_out=out):
        return lib.qecmc_class_sample_tiled(code, L, n, L_.u8(chains), None if weights is None else weights.ctypes.data_as(_f64p), hbm_width, tile_width, record_bytes, K,
                                            SEED, 0, mode, None if chain_out is None else L_.u8(chain_out), L_.i32(cls), z.ctypes.data_as(_f64p))
    for args, rc_want, want in [((ROTATED, 13, 1, w, 0, 3), INVALID, "tile_width=3"), ((ROTATED, 13, 1, w, 25, 0), INVALID, "hbm_width=25"),
                                ((TORIC, 4, 1, w), UNSUPPORTED, ""), ((ROTATED, 13, 1, None), INVALID, "NULL buffer"),
                                ((ROTATED, 13, 1, w, 0, 0, 0, 1, 0, None), INVALID, "NULL buffer"), ((ROTATED, 13, 1 << 32, w), INVALID, "exceed 32 bits"),
                                ((ROTATED, 13, 1, w, 0, 0, 0, 0), INVALID, "K=0"), ((ROTATED, 13, 1, w, 0, 0, 0, 1, 3), INVALID, "mode=3"),
                                ((ROTATED, 13, 1, w, 0, 0, CAP_MAX + 1), INVALID, "record_bytes="),
                                ((ROTATED, 21, 1, w), UNSUPPORTED, "%d bytes" % (128 * 303650944)),          # refused at the default cap without a device call
                                ((ROTATED, 13, 1, w, 0, 0, 1 << 20), UNSUPPORTED, "%d bytes" % (128 * 496896))]:
        assert call(*args) == rc_want, args                                     # before a device is looked for: this machine may have none
        msg = lib.qecmc_last_error().decode()
        assert msg.startswith(PREFIX) and want in msg, msg
    site = lib.qecmc_class_sample_tiled_site
    tail = (0, 0, 0, 1, SEED, 0, 0, L_.u8(out), L_.i32(cls), z.ctypes.data_as(_f64p))
    assert site(ROTATED, 13, 1, L_.u8(chains), None, 1, *tail) == INVALID and lib.qecmc_last_error().decode() == SITE_PREFIX + "NULL buffer"
    wq = np.ones((2, 169, 4))
    assert site(ROTATED, 13, 3, L_.u8(np.zeros((3, 169), np.uint8)), wq.ctypes.data_as(_f64p), 2, *tail) == INVALID
    assert lib.qecmc_last_error().decode().startswith(SITE_PREFIX + "wq_rows=2")
    # the info call: the plan's numbers from the host half alone, and the refusal for the cap with the numbers still written
    nf, b, j = C.c_int32(), C.c_uint64(), C.c_uint32()
    assert lib.qecmc_class_sample_tiled_info(ROTATED, 13, 0, 0, 0, C.byref(nf), C.byref(b), C.byref(j)) == 0
    assert (nf.value, b.value, j.value) == (168, 128 * 496896, 67)
    assert lib.qecmc_class_sample_tiled_info(ROTATED, 13, 0, 0, 3 * b.value, None, None, C.byref(j)) == 0 and j.value == 3
    assert lib.qecmc_class_sample_tiled_info(ROTATED, 21, 0, 0, 0, C.byref(nf), C.byref(b), None) == UNSUPPORTED and b.value == 128 * 303650944 and nf.value == 440
    assert "qecmc_class_sample_tiled_info: " in lib.qecmc_last_error().decode()
    assert lib.qecmc_class_sample_tiled_info(ROTATED, 21, 0, 0, 40 << 30, None, None, C.byref(j)) == 0 and j.value == 1
    # N == 0 succeeds where a device is there, and asks for one where none is: every refusal above came first
    assert call(ROTATED, 13, 0, w) == (0 if lib.qecmc_device_count() > 0 else NO_DEVICE)


# ------------------------------------------------------------------------------------------------------ the Python layer
class FakeLib:
    """qecmc_class_sample_tiled(_site) answered by the twin: the Python layer around them, without a device"""
    def __init__(self, T):
        self.T, self.real, self.calls = T, L_.lib(), []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def qecmc_class_sample_tiled(self, code, L, n, chains, w, hbm_width, tile_width, record_bytes, K, seed, first, mode, chain_out, cls, z):
        self.calls.append(("uniform", code, L, n, hbm_width, tile_width, record_bytes, mode))
        return self.T.qt_class_sample_tiled(code, L, n, C.cast(chains, _u8p), w, None, 0, hbm_width, tile_width, record_bytes, K, seed, first, mode, C.cast(chain_out, _u8p),
                                            C.cast(cls, _i32p), z, None, 0)

    def qecmc_class_sample_tiled_site(self, code, L, n, chains, wq, rows, hbm_width, tile_width, record_bytes, K, seed, first, mode, chain_out, cls, z):
        self.calls.append(("site", code, L, n, hbm_width, tile_width, record_bytes, mode))
        return self.T.qt_class_sample_tiled(code, L, n, C.cast(chains, _u8p), None, wq, rows, hbm_width, tile_width, record_bytes, K, seed, first, mode,
                                            C.cast(chain_out, _u8p), C.cast(cls, _i32p), z, None, 0)


def test_python_layer_shapes_keys_and_routes(T, monkeypatch):
    fake = FakeLib(T)
    monkeypatch.setattr(L_, "lib", lambda: fake)
    chains = MT.chains_of(ROTATED, 7, 3, seed=12)
    r = ex.sample_chains_tiled("rotated", chains, w4=BIASED, n_samples=4, seed=SEED, first_syndrome=5, tile_width=5)
    out, _, z = twin(T, ROTATED, 7, chains, w=BIASED, K=4, first=5, tile_width=5)
    assert set(r) == {"chains", "z", "width", "held"} and r["chains"].shape == (3, 4, 4, 7, 7) and r["chains"].dtype == np.uint8
    assert np.array_equal(r["chains"].reshape(out.shape), out) and r["z"].tobytes() == z.tobytes()
    assert (r["width"], r["held"]) == (ST.info(T, ROTATED, 7, 0, 5)[1]["width"], 0)
    assert np.array_equal(ex.sample_chains_tiled("rotated", chains, p=0.1, eta=10.0, n_samples=4, seed=SEED, first_syndrome=5, tile_width=5)["chains"], r["chains"])
    tabs = np.random.default_rng(3).uniform(0.1, 1.0, size=(3, 7, 7, 4))
    rs = ex.sample_chains_tiled_site("rotated", chains, tabs, n_samples=2, seed=SEED, tile_width=5, record_bytes=1 << 30)
    assert np.array_equal(rs["chains"].reshape(3, 4, 2, 49), twin(T, ROTATED, 7, chains, wq=tabs.reshape(3, 49, 4), K=2, tile_width=5)[0])
    post = ex.sample_posterior("rotated", chains, w4=BIASED, n_samples=4, seed=SEED, first_syndrome=5, method="tiled", tile_width=5)
    want, cls, _ = twin(T, ROTATED, 7, chains, w=BIASED, K=4, first=5, mode=1, tile_width=5)
    assert set(post) == {"chains", "cls", "z", "width", "held"} and post["chains"].shape == (3, 4, 7, 7)
    assert np.array_equal(post["chains"].reshape(want.shape), want) and np.array_equal(post["cls"], cls)
    site_post = ex.sample_posterior("rotated", chains, site_weights=tabs, n_samples=2, seed=SEED, method="tiled", tile_width=5)
    assert np.array_equal(site_post["chains"].reshape(3, 2, 49), twin(T, ROTATED, 7, chains, wq=tabs.reshape(3, 49, 4), K=2, mode=1, tile_width=5)[0])
    counts = ex.posterior_error_counts("rotated", chains, 0.1, 16, seed=SEED, method="tiled", tile_width=5)
    drawn = twin(T, ROTATED, 7, chains, w=ex.depolarizing_w4(0.1), K=16, mode=1, tile_width=5)[0]
    assert counts.shape == (3,) and np.array_equal(counts, np.count_nonzero(drawn, axis=2).mean(axis=1))
    assert [c[0] for c in fake.calls] == ["uniform", "uniform", "site", "uniform", "site", "uniform"] and all(c[5] == 5 for c in fake.calls)
    assert [c[6] for c in fake.calls] == [0, 0, 1 << 30, 0, 0, 0] and [c[7] for c in fake.calls] == [0, 0, 0, 1, 1, 1]
    # a width of the other route is refused by name, as min_weight_corrections refuses it; the default stays the cut route
    with pytest.raises(ValueError, match="lds_width belongs to method='cut'"):
        ex.sample_posterior("rotated", chains, p=0.1, method="tiled", lds_width=13)
    with pytest.raises(ValueError, match="hbm_width, tile_width and record_bytes belong to method='tiled'"):
        ex.sample_posterior("rotated", chains, p=0.1, tile_width=5)
    with pytest.raises(ValueError, match="hbm_width, tile_width and record_bytes belong to method='tiled'"):
        ex.posterior_error_counts("rotated", chains, 0.1, 4, record_bytes=1 << 30)
    with pytest.raises(ValueError, match="method='auto'"):
        ex.sample_posterior("rotated", chains, p=0.1, method="auto")
    with pytest.raises(ValueError, match="n_samples"):
        ex.sample_chains_tiled("rotated", chains, p=0.1, n_samples=0)
    with pytest.raises(ValueError, match="either p"):
        ex.sample_chains_tiled("rotated", chains)
    import qecmc
    assert qecmc.sample_chains_tiled is ex.sample_chains_tiled and qecmc.sample_chains_tiled_site is ex.sample_chains_tiled_site
    assert qecmc.sample_tiled_info is ex.sample_tiled_info


def test_python_layer_refuses_before_a_device_is_looked_for():
    with pytest.raises(L_.QecmcError, match="qecmc_class_sample_tiled: .*no class move"):
        ex.sample_chains_tiled("toric", np.zeros((1, 2, 4, 4), np.uint8), p=0.1)
    with pytest.raises(L_.QecmcError, match="qecmc_class_sample_tiled_site: tile_width=3"):
        ex.sample_chains_tiled_site("rotated", np.zeros((1, 13, 13), np.uint8), np.ones((13, 13, 4)), tile_width=3)
    with pytest.raises(L_.QecmcError, match="qecmc_class_sample_tiled: .*%d bytes" % (128 * 303650944)):
        ex.sample_posterior("rotated", np.zeros((1, 21, 21), np.uint8), p=0.1, method="tiled")
    with pytest.raises(L_.QecmcError, match="%d bytes" % (128 * 77956992)):
        ex.sample_tiled_info("toric", 7)
    assert ex.sample_tiled_info("rotated", 17) == dict(n_forget=288, bytes_per_job=128 * 13082880, jobs_per_pass=2)
    assert ex.sample_tiled_info("rotated", 21, record_bytes=40 << 30)["jobs_per_pass"] == 1
