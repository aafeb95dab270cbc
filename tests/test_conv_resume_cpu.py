"""Criterion runs continued from device state (qecmc_pteq_resume_conv_dev), the parts that need no GPU: the entry points exist and refuse
what they must, the one host formula of the record and log sizes (csrc/plan_host.hpp resume_conv_need) against values written out by hand, the
kernel choice of a continued launch, and harness.LadderRun's log-growth arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hostlib import ROOT, tables_lib
from qecmc import _lib as L_
from qecmc import harness

INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -4
NEW = ("qecmc_pteq_resume_conv_dev", "qecmc_plan_resume_conv_bytes")


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_resume_conv_bytes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.qt_resume_conv_bytes.restype = None
    lib.qt_resume_conv_check.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    return lib


def params(**kw):
    return L_.make_params(**dict(dict(p=0.1, eta=3.0, alpha=1.5, iters=10, steps=10, p_logical=0.5), **kw))


def test_header_library_and_binding_carry_the_entry_points():
    header = open(os.path.join(ROOT, "include", "qecmc.h")).read()
    lib = L_.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L_.SIGNATURES and hasattr(lib, name)
    assert len(L_.SIGNATURES["qecmc_pteq_resume_conv_dev"][1]) == 18 and len(L_.SIGNATURES["qecmc_plan_resume_conv_bytes"][1]) == 5
    assert lib.qecmc_abi_version() == 4                                # additive: the ABI version stays


def test_null_plan_is_invalid_and_no_plan_exists_without_a_device():
    """(The entry point's own QECMC_ERR_NO_DEVICE answer needs a plan, and a plan needs a device: it cannot be reached on a machine without one.)"""
    lib = L_.lib()
    rec, log = C.c_uint64(), C.c_uint64()
    assert lib.qecmc_pteq_resume_conv_dev(None, None, None, None, 64, 0, 0, None, None, None, None, None, 0, None, None, 0, 0, None) == INVALID
    assert b"plan" in lib.qecmc_last_error()
    assert lib.qecmc_plan_resume_conv_bytes(None, 64, 10, C.byref(rec), C.byref(log)) == INVALID
    if lib.qecmc_device_count() == 0:
        # the only way to a plan is qecmc_plan_create, which answers for every compute entry point on a machine without a device
        plan = C.c_void_p()
        assert lib.qecmc_plan_create(params(code=L_.TORIC, L=5, Nc=5, conv_mode=L_.CONV_ERROR_BASED), C.byref(plan)) == NO_DEVICE
        assert not plan.value


# (code, noise, N, log_rows) -> (record bytes, log bytes), by hand: 48 B per ladder (alpha rule: 64 B); 2 B (alpha: 4 B) x ceil64(N) x log_rows
SIZES = [
    (L_.TORIC, L_.NOISE_DEPOLARIZING, 64, 100, 48 * 64, 2 * 64 * 100),
    (L_.TORIC, L_.NOISE_DEPOLARIZING, 65, 100, 48 * 65, 2 * 128 * 100),
    (L_.TORIC, L_.NOISE_DEPOLARIZING, 1, 1 << 20, 48, 2 * 64 * (1 << 20)),
    (L_.XZZX, L_.NOISE_BIASED, 200, 7, 48 * 200, 2 * 256 * 7),
    (L_.ROTATED, L_.NOISE_ALPHA, 200, 7, 64 * 200, 4 * 256 * 7),
    (L_.XZZX, L_.NOISE_ALPHA, 63, 1, 64 * 63, 4 * 64 * 1),
    (L_.ROTATED, L_.NOISE_DEPOLARIZING, 1000, 0, 48 * 1000, 0),
]


@pytest.mark.parametrize("code,noise,N,rows,rec_exp,log_exp", SIZES)
def test_record_and_log_sizes_by_hand(T, code, noise, N, rows, rec_exp, log_exp):
    rec, log = C.c_uint64(), C.c_uint64()
    for steps in (1, 999):                                             # the sizes do not depend on the chunk length of the plan
        T.qt_resume_conv_bytes(C.byref(params(code=code, L=5, Nc=5, noise=noise, conv_mode=L_.CONV_ERROR_BASED, steps=steps)), N, rows, C.byref(rec), C.byref(log))
        assert (rec.value, log.value) == (rec_exp, log_exp)
    T.qt_resume_conv_bytes(C.byref(params(code=code, L=5, Nc=5, noise=noise)), N, rows, C.byref(rec), C.byref(log))
    assert (rec.value, log.value) == (0, 0)                            # no criterion, nothing to carry


def test_plans_refused_before_any_buffer_is_looked_at(T):
    msg = C.create_string_buffer(600)
    ok = dict(code=L_.TORIC, L=5, Nc=5, conv_mode=L_.CONV_ERROR_BASED)
    assert T.qt_resume_conv_check(C.byref(params(**ok)), msg, len(msg)) == 0
    assert T.qt_resume_conv_check(C.byref(params(**dict(ok, scan=L_.SCAN_SWEEP))), msg, len(msg)) == 0
    assert T.qt_resume_conv_check(C.byref(params(**dict(ok, replicas=1))), msg, len(msg)) == 0
    assert T.qt_resume_conv_check(C.byref(params(**dict(ok, conv_mode=L_.CONV_NONE))), msg, len(msg)) == INVALID and b"conv_mode" in msg.value
    assert T.qt_resume_conv_check(C.byref(params(**dict(ok, scan=L_.SCAN_WAVE))), msg, len(msg)) == UNSUPPORTED and b"wave" in msg.value
    assert T.qt_resume_conv_check(C.byref(params(**dict(ok, scan=L_.SCAN_COLOUR))), msg, len(msg)) == UNSUPPORTED and b"colour" in msg.value
    assert T.qt_resume_conv_check(C.byref(params(**dict(ok, replicas=2))), msg, len(msg)) == INVALID and b"replicas" in msg.value


def test_a_continued_launch_runs_the_kernel_of_a_fresh_one(T):
    """choose_kernel() for conv = 1, resume = 1, queue = 0 on scan 0 / 1 is the key of resume = 0: no new instantiation.  (The launch also sets
    QECMC_FLAG_NO_PRE, a developer switch between equivalent variants: the key then is the one resume = 0 has under the same switch.)"""
    import test_kernel_choice as tk
    shapes = []
    for code in (L_.TORIC, L_.XZZX, L_.ROTATED, L_.PLANAR):
        for noise, scan in ((0, 0), (0, 1), (1, 0), (2, 0)):
            if noise and code in (L_.TORIC, L_.PLANAR):
                continue
            for L in (3, 5, 9, 15):
                for Nc in (1, 3, 8, 12):
                    for flags in (0, L_.FLAG_NO_PRE):
                        rc, _, shape, _, _ = tk.plan(T, params(code=code, L=L, Nc=Nc, noise=noise, scan=scan, conv_mode=L_.CONV_ERROR_BASED, flags=flags))
                        if rc == 0:
                            shapes.append([shape[f] for f in tk.FIELDS])
    assert len(shapes) > 200
    fresh = np.array(shapes, dtype=np.int32)
    assert (fresh[:, tk.FIELDS.index("conv")] == 1).all() and (fresh[:, tk.FIELDS.index("queue")] == 0).all()
    cont = fresh.copy()
    cont[:, tk.FIELDS.index("resume")] = 1
    cont[:, tk.FIELDS.index("neff")] = fresh[:, tk.FIELDS.index("noise")] == 2      # the alpha rule's continuation passes d_neff
    ka, kb = np.zeros((len(fresh), 11), dtype=np.int64), np.zeros((len(fresh), 11), dtype=np.int64)
    T.qt_choose_kernels(fresh.ctypes.data, len(fresh), ka.ctypes.data)
    T.qt_choose_kernels(cont.ctypes.data, len(cont), kb.ctypes.data)
    assert np.array_equal(ka[:, :10], kb[:, :10]) and (ka[:, 0] == 1).all()          # ladder kernels, the same ones
    no_pre = fresh[:, tk.FIELDS.index("tune")] & L_.FLAG_NO_PRE != 0
    assert no_pre.any() and not (ka[no_pre, 4] & (1 << tk.FLAGS.index("pre"))).any()  # what a continued launch runs is never a PRE kernel


def test_log_growth_arithmetic():
    g = harness.grown_log_rows
    assert g(100, 0, 100) == (100, 0) and g(100, 40, 60) == (100, 0)                  # fits: nothing to do
    assert g(100, 100, 1) == (200, 100)                                               # geometric: twice the rows, all written rows carried
    assert g(100, 60, 41) == (200, 60)
    assert g(100, 100, 500) == (600, 100)                                             # ... or as many as the chunk needs
    assert g(1, 0, 7) == (7, 0)                                                       # nothing written yet: nothing to copy
    assert g(64, 64, 64, growth=16) == (1024, 64)
    rows, steps = 16, 0
    for chunk in (1, 15, 1, 40, 1000):                                                # a run: the log always holds the chunk, rows only ever grow
        new, keep = g(rows, steps, chunk)
        assert new >= steps + chunk and new >= rows and keep == (steps if new != rows else 0)
        rows, steps = new, steps + chunk


def test_packed_neff_counts():
    st = np.array([[0, 1, 2, 3, 3, 0], [3, 3, 3, 3, 3, 3]], dtype=np.uint8)
    assert harness.packed_neff(st).tolist() == [2 | (2 << 16), 6]
