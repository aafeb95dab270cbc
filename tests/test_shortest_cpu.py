"""The shortest-chain statistics of PTEQ_alpha_with_shortest in the kernels (qecmc_plan_set_shortest, qecmc.pteq_shortest_batch), as far as a machine
without a GPU can tell: the entry points exist and refuse, before they look for a device, what they must; qecmc.shortest_distribution -- a pure host
function -- turns the raw arrays of the CPU twin (tests/util_shortest_batch.py, level (i)) into the three vectors of the reference's host loop (level
(ii)); the chooser routes stats = 2 to kernels that are in the build, and those use no scratch; the set workspace follows its one formula."""
import ctypes as C
import importlib.util
import inspect
import os

import numpy as np
import pytest

import util_shortest_batch as U
from hostlib import ROOT, resource_rows, tables_lib

ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_shortest_check.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.qt_shortest_set_need.argtypes = [C.c_uint64, C.c_uint64]
    lib.qt_shortest_set_need.restype = C.c_uint64
    return lib


def params(**kw):
    from qecmc import _lib as L_
    base = dict(code=L_.XZZX, L=5, Nc=5, p=0.2, p_logical=0.5, iters=10, steps=100, tops_burn=1, noise=L_.NOISE_ALPHA, alpha=2.0, scan=L_.SCAN_WAVE)
    base.update(kw)
    return L_.make_params(**base)


def batch_call(pr, N=2, null=None, set_capacity=1024):
    """qecmc_pteq_batch_shortest on host buffers of N ladders; `null`: the argument passed as NULL -> (return code, message)"""
    from qecmc import _lib as L_
    lib = L_.lib()
    bufs = dict(init=np.zeros((N, pr.L, pr.L), np.uint8), counts=np.zeros((N, 4), np.uint32), samples=np.zeros(N, np.uint32), tops0=np.zeros(N, np.uint32),
                steps_done=np.zeros(N, np.uint32), converged=np.zeros(N, np.uint8), shortest=np.zeros((N, 4)), shortest_n=np.zeros((N, 4), np.uint32),
                unique_n=np.zeros((N, 4), np.uint32), overflow=np.zeros(N, np.uint8))
    ptr = {k: None if k == null else v.ctypes.data_as(C.c_void_p) for k, v in bufs.items()}
    cast = lambda k, t: C.cast(ptr[k], t) if ptr[k] is not None else None
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    rc = lib.qecmc_pteq_batch_shortest(pr, cast("init", u8), N, set_capacity, cast("counts", u32), cast("samples", u32), cast("tops0", u32),
                                       cast("steps_done", u32), cast("converged", u8), cast("shortest", C.POINTER(C.c_double)), cast("shortest_n", u32),
                                       cast("unique_n", u32), cast("overflow", u8), None)
    return rc, lib.qecmc_last_error().decode()


def test_the_entry_points_exist():
    import qecmc
    from qecmc import _lib as L_
    lib = L_.lib()
    for name in ("qecmc_plan_set_shortest", "qecmc_plan_shortest_set_bytes", "qecmc_pteq_batch_shortest"):
        assert hasattr(lib, name) and name in L_.SIGNATURES
    assert lib.qecmc_abi_version() == 4
    assert callable(qecmc.pteq_shortest_batch) and callable(qecmc.shortest_distribution)
    sig = inspect.signature(qecmc.pteq_shortest_batch).parameters
    assert sig["set_capacity"].default == 1024 and "scan" in sig and "conv_criteria" in sig and "first_syndrome" in sig
    assert inspect.signature(qecmc.PTEQ_alpha_with_shortest).parameters["scan"].default == "random"


def test_refusals_come_before_the_device_with_their_codes_and_texts():
    from qecmc import _lib as L_
    rc, msg = batch_call(params(noise=L_.NOISE_DEPOLARIZING, p=0.1))
    assert rc == ERR_UNSUPPORTED and "qecmc_plan_set_shortest: shortest-chain statistics: the alpha rule only" in msg, (rc, msg)
    rc, msg = batch_call(params(scan=L_.SCAN_RANDOM))
    assert rc == ERR_UNSUPPORTED and "scan = wave or scan = colour" in msg, (rc, msg)
    rc, msg = batch_call(params(replicas=2))
    assert rc == ERR_UNSUPPORTED and "not with replicas > 1" in msg, (rc, msg)
    for scan in (L_.SCAN_WAVE, L_.SCAN_COLOUR):
        for null in ("init", "counts", "samples", "shortest", "shortest_n", "unique_n", "overflow"):
            rc, msg = batch_call(params(scan=scan), null=null)
            assert rc == ERR_INVALID and "NULL buffer" in msg, (scan, null, rc, msg)
        rc, msg = batch_call(params(scan=scan), set_capacity=0)
        assert rc == ERR_INVALID and "set_capacity" in msg, (rc, msg)
    lib = L_.lib()
    assert lib.qecmc_plan_set_shortest(None, None, None, None, None, None, 0, 1024) == ERR_INVALID
    out = C.c_uint64(0)
    assert lib.qecmc_plan_shortest_set_bytes(None, 4, 1024, C.byref(out)) == ERR_INVALID


def test_the_host_check_names_each_case(T):
    from qecmc import _lib as L_
    msg = C.create_string_buffer(600)
    for kw, code, text in ((dict(), 0, ""), (dict(scan=L_.SCAN_COLOUR), 0, ""), (dict(code=L_.ROTATED, Nc=9), 0, ""),
                           (dict(noise=L_.NOISE_DEPOLARIZING, p=0.1), ERR_UNSUPPORTED, "the alpha rule only"),
                           (dict(noise=L_.NOISE_BIASED, eta=10.0, scan=L_.SCAN_COLOUR), ERR_UNSUPPORTED, "the alpha rule only"),
                           (dict(scan=L_.SCAN_RANDOM), ERR_UNSUPPORTED, "scan = wave or scan = colour"),
                           (dict(replicas=2), ERR_UNSUPPORTED, "not with replicas > 1"),
                           (dict(L=13), ERR_UNSUPPORTED, "scan = wave")):                        # 11 words: beyond the alpha rule's wave kernels
        rc = T.qt_shortest_check(C.byref(params(**kw)), msg, len(msg))
        assert rc == code and text in msg.value.decode(), (kw, rc, msg.value)


def test_set_bytes_formula(T):
    # slots: the smallest power of two >= 2 x capacity; 8 bytes each; one table per ladder
    assert T.qt_shortest_set_need(70, 1024) == 70 * 2048 * 8 == 1146880
    assert T.qt_shortest_set_need(3, 8) == 3 * 16 * 8 == 384
    assert T.qt_shortest_set_need(1, 1000) == 2048 * 8 and T.qt_shortest_set_need(1, 1025) == 4096 * 8 and T.qt_shortest_set_need(5, 1) == 5 * 2 * 8


def test_the_lds_request_holds_the_statistics_state(T):
    """The shortest-chain kernels keep kShortRows words per ladder in LDS beyond the plain kernels' map: the bytes a launch asks for (and
    qecmc_plan_info reports while the statistics are set) exceed the plan's plain figure by at least that, and on scan = colour, where the kernel
    places the words itself (colour_short_at, the offset ladder_colour_body.inc uses), their last word lies inside the request"""
    from qecmc import _lib as L_
    T.qt_shortest_lds.argtypes = [C.c_void_p] * 5
    sb, pb, at, rows = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    seen_odd = set()
    for code, L in ((L_.XZZX, 3), (L_.XZZX, 5), (L_.XZZX, 7), (L_.XZZX, 9), (L_.ROTATED, 3), (L_.ROTATED, 5), (L_.ROTATED, 9)):
        for Nc in (2, 3, 4, 5, 8, 9, 12, 16):
            for scan in (L_.SCAN_COLOUR, L_.SCAN_WAVE):
                for conv in (L_.CONV_NONE, L_.CONV_ERROR_BASED):
                    pr = params(code=code, L=L, Nc=Nc, scan=scan, conv_mode=conv)
                    assert T.qt_shortest_lds(C.byref(pr), C.byref(sb), C.byref(pb), C.byref(at), C.byref(rows)) == 0, (code, L, Nc, scan)
                    assert rows.value == 18
                    per = rows.value * (64 if scan == L_.SCAN_WAVE else 1)            # (wave: a row per lane)
                    assert sb.value <= 160 * 1024
                    # (a fixed-length wave plan pads its exchange rows, the shortest-chain kernels -- criterion kernels -- do not: compare like with like)
                    if scan == L_.SCAN_COLOUR or conv == L_.CONV_ERROR_BASED:
                        assert sb.value >= pb.value + 4 * per, (code, L, Nc, scan, sb.value, pb.value)
                    if scan == L_.SCAN_COLOUR:
                        assert 4 * (at.value + rows.value) <= sb.value, (code, L, Nc, at.value, sb.value)
                        assert 4 * at.value >= pb.value - 16, (code, L, Nc, at.value, pb.value)   # behind everything else (the plain map ends in <= 4 spare words)
                        seen_odd.add(at.value & 1)
    assert seen_odd == {0, 1}


TWINS = [("xzzx", 3, 3, 70, 250, 10, 0.3, 2.0, "wave", True, 2, 4, 2, 0.6, 31, 64), ("xzzx", 3, 3, 70, 250, 10, 0.3, 2.0, "colour", True, 2, 4, 2, 0.6, 31, 64),
         ("rotated", 5, 4, 6, 300, 7, 0.2, 1.7, "wave", False, 2, 10, 1, 0.1, 31, 0)]


@pytest.mark.parametrize("args", TWINS, ids=["A-wave", "A-colour", "rotated-noninteger-alpha"])
def test_shortest_distribution_equals_the_host_loop(args):
    """level (i) -> shortest_distribution == level (ii): first vector exact, the others at rtol = 1e-9 (k x term against k sequential additions: at most
    k 2^-53 apart, k <= 2^20), NaN positions equal"""
    import qecmc
    raw = dict(U.raw(*args))
    raw["overflow"] = np.zeros(len(raw["samples"]), dtype=bool)
    a, b, c = qecmc.shortest_distribution(raw, args[6])
    ra, rb, rc = U.triple(*args)
    assert a.dtype == np.uint8 and a.shape == ra.shape and np.array_equal(a, ra)
    assert b.dtype == np.float64 and c.dtype == np.float64
    np.testing.assert_allclose(b, rb, rtol=1e-9, atol=0, equal_nan=True)
    np.testing.assert_allclose(c, rc, rtol=1e-9, atol=0, equal_nan=True)
    assert np.isfinite(rb).all(axis=1).sum() >= 2 and (raw["unique_n"].max(axis=1) >= 2).any()      # (ladders that never left burn-in: NaN rows on both sides)
    # an overflowed ladder: its second vector is NaN, nothing else moves
    raw["overflow"] = raw["overflow"].copy()
    raw["overflow"][1] = True
    a2, b2, c2 = qecmc.shortest_distribution(raw, args[6])
    assert np.isnan(b2[1]).all() and np.array_equal(np.delete(b2, 1, axis=0), np.delete(b, 1, axis=0), equal_nan=True) and np.array_equal(a2, a) and \
        np.array_equal(c2, c, equal_nan=True)


def test_a_ladder_that_never_left_burn_in_divides_by_zero_like_the_reference():
    import qecmc
    from qecmc.decoders_biasednoise import _shortest_loop
    # the reference's loop on a ladder whose tops0 never reaches tops_burn
    ld = U.OracleLadder(U.CODE["xzzx"], U.make_init(5, 5, 1)[0], 0.2, 2.0, 5, 3, U.orc.Rng.philox(1, 0))
    ra, rb, rc = _shortest_loop(ld, 0.2, 2, 10, 10 ** 6, 0.1, 20, 10, None)
    res = dict(counts=np.zeros((1, 4), np.uint32), samples=np.zeros(1, np.uint32), shortest=np.full((1, 4), 100000.0), shortest_n=np.zeros((1, 4), np.uint32),
               unique_n=np.zeros((1, 4), np.uint32), overflow=np.zeros(1, bool))
    a, b, c = qecmc.shortest_distribution(res, 0.2)
    assert np.array_equal(a[0], ra) and np.isnan(rb).all() and np.isnan(b).all() and np.isnan(rc).all() and np.isnan(c).all()


@pytest.fixture(scope="module")
def built():
    return {r["label"]: r for r in resource_rows() if r["label"].startswith(("wave-shortest<", "colour-shortest<"))}


WANT = {"wave-shortest<1024,4,%s: %d words%s>" % (c, w, it) for c in ("xzzx", "rotated") for w in (4, 8) for it in ("", ", iters 10")} | \
       {"colour-shortest<1024,4,%s>" % c for c in ("xzzx", "rotated")}


def test_the_shortest_kernels_are_built_without_scratch(built):
    assert set(built) == WANT
    for lab, r in sorted(built.items()):
        print("%-52s VGPRs %3d  SGPRs %3d  scratch %d  occupancy %d" % (lab, r["VGPRs"], r["SGPRs"], r["ScratchSize"], r["Occupancy"]))
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 128 and r["Occupancy"] >= 4, r
        assert r["unit"] in ("ladder_wu_shortest", "ladder_colour_shortest"), r
        assert "ladder_wu_kernelI" not in r["kernel"] and "ladder_colour_kernelI" not in r["kernel"], r


def test_the_chooser_routes_stats_2_to_built_kernels_and_leaves_the_rest(T, built):
    from qecmc import _lib as L_
    KC = _load("test_kernel_choice", os.path.join(ROOT, "tests", "test_kernel_choice.py"))
    FIELDS, CODES = KC.FIELDS, KC.CODES
    dims, msg = np.zeros(len(FIELDS), dtype=np.int32), C.create_string_buffer(600)
    rows, want = [], []
    for code, L, Nc, iters, scan in ((L_.XZZX, 3, 3, 10, 3), (L_.XZZX, 9, 8, 10, 3), (L_.ROTATED, 5, 4, 7, 3), (L_.ROTATED, 5, 9, 10, 3), (L_.XZZX, 7, 16, 1, 3),
                                     (L_.XZZX, 5, 5, 10, 2), (L_.ROTATED, 9, 12, 10, 2)):
        assert T.qt_plan_dims(C.byref(params(code=code, L=L, Nc=Nc, iters=iters, scan=scan)), dims.ctypes.data, msg, len(msg)) == 0, msg.value
        for conv in (0, 1):
            for stats in (0, 2):
                s = dict(zip(FIELDS, (int(x) for x in dims)))
                s.update(Nc=Nc, top_acc=0 if scan == 3 else 1, lower_acc=0, logical=1, conv=conv, queue=0, uset=0, xyz=0, stats=stats, resume=0, neff=0, f32ok=1,
                         swap_fast_ok=1, iters=iters, tune=0)
                rows.append([s[f] for f in FIELDS])
                W = (L * L + 15) // 16
                want.append(None if not stats else "colour-shortest<1024,4,%s>" % CODES[code] if scan == 2 else
                            "wave-shortest<1024,4,%s: %d words%s>" % (CODES[code], 4 if W <= 4 else 8, ", iters 10" if iters == 10 else ""))
    shapes = np.ascontiguousarray(rows, dtype=np.int32)
    keys = np.zeros((len(shapes), 11), dtype=np.int64)
    T.qt_choose_kernels(shapes.ctypes.data, len(shapes), keys.ctypes.data)
    for s, k, w in zip(rows, keys, want):
        family, maxt, minw, code, flags, wv, conv, it, alpha, rule, _ = (int(x) for x in k)
        assert family in (2, 3), (s, k)
        if w is None:
            assert flags == 0, (s, k)                       # stats = 0: the fast kernels' keys
            continue
        assert (flags, maxt, minw, conv) == (2, 1024, 4, 1), (s, k)
        lab = "colour-shortest<1024,4,%s>" % CODES[code] if family == 3 else "wave-shortest<1024,4,%s: %d words%s>" % (CODES[code], wv, ", iters 10" if it else "")
        assert lab == w and lab in built, (s, lab, w)
    # resumed ladders are refused by name
    s = dict(zip(FIELDS, rows[1]))
    s["resume"] = 1
    one = np.ascontiguousarray([[s[f] for f in FIELDS]], dtype=np.int32)
    T.qt_choose_kernels(one.ctypes.data, 1, keys.ctypes.data)
    assert keys[0][0] == 0 and C.string_at(int(keys[0][10])).decode() == "shortest-chain statistics: no resumed ladders"
