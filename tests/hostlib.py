"""The tests' plumbing for what the build leaves on the host, in one place: the g++-built host test API (csrc/tables_test_api.cpp, `make tables`), KernelShape
rows for the choice functions it exports, the build's resource tables (csrc/build/<unit>.res through tools/kernel_resources.py) and the stand-alone
sanitizer self-tests.  A helper module beside kernel_cases.py and util_exact.py: no tests, no fixtures."""
import ctypes as C
import functools
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc")
for _p in (ROOT, os.path.join(ROOT, "mcmc-qec-toric-rl_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from qecmc import _lib as L_            # noqa: E402

TORIC, XZZX, ROTATED, PLANAR = 0, 1, 2, 3
# the label heads of the sealed registry: the ladder / wave / colour / statistics / shortest-chain kernels tests/kernel_cases.json enumerates
SEALED_HEADS = ("ladder<", "wave<", "colour<", "wave-stats<", "colour-stats<", "wave-shortest<", "colour-shortest<")
# KernelShape (csrc/kernel_choice.hpp), field by field
KERNEL_SHAPE_FIELDS = ["code", "noise", "scan", "L", "Nc", "W", "nq", "ncls", "n_gen", "n_types", "gen_type", "top_acc", "lower_acc", "logical", "conv",
                       "queue", "uset", "xyz", "stats", "resume", "neff", "f32ok", "swap_fast_ok", "iters", "tune"]


# ------------------------------------------------------------------------------------------------------------------ the host test API
@functools.lru_cache(maxsize=None)
def _tables_lib(path):
    if not path:
        subprocess.check_call(["make", "-C", CSRC, "-s", "tables"])
        path = os.path.join(CSRC, "build", "libqecmc_tables.so")
    lib = C.CDLL(path)
    assert lib.qt_kernel_shape_ints() == len(KERNEL_SHAPE_FIELDS)
    lib.qt_plan_dims.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.qt_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.qt_choose_kernels.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.qt_launch_takes_queue.argtypes = [C.c_uint32, C.c_uint64, C.c_int]
    return lib


def tables_lib():
    """the g++-built host test API (csrc/tables_test_api.cpp): the library QECMC_TABLES_LIB names -- how the sanitizer child of tests/test_host_tables.py
    hands its build to every module -- or `make tables`; one CDLL per path, with the argtypes of the shape functions every caller shares"""
    return _tables_lib(os.environ.get("QECMC_TABLES_LIB") or "")


# ------------------------------------------------------------------------------------------------------------------ KernelShape rows
_DIMS = {}


def launch_shape(T, code, L, Nc, noise=0, scan=3, **kw):
    """the KernelShape row of a fixed-length launch of the plan of (code, L, rule, scan) with Nc rungs: the static fields from plan_dims() (asked once per
    plan), the ladder's as tests/test_kernel_choice.py bench_shape() sets them (depolarizing rule: a top rung at p = 0.75 over distinct temperatures)"""
    if (code, L, noise, scan) not in _DIMS:
        dims, msg = np.zeros(len(KERNEL_SHAPE_FIELDS), dtype=np.int32), C.create_string_buffer(600)
        pr = L_.make_params(p=0.1, eta=3.0, alpha=1.5, iters=10, steps=10, code=code, L=L, Nc=2, noise=noise, scan=scan)
        assert T.qt_plan_dims(C.byref(pr), dims.ctypes.data, msg, len(msg)) == 0, msg.value
        _DIMS[(code, L, noise, scan)] = dict(zip(KERNEL_SHAPE_FIELDS, (int(x) for x in dims)))
    s = dict(_DIMS[(code, L, noise, scan)])
    s.update(Nc=Nc, top_acc=int(noise == 0), lower_acc=0, logical=1, conv=0, queue=0, uset=0, xyz=0, stats=0, resume=0, neff=0, f32ok=int(noise == 2),
             swap_fast_ok=1, iters=10, tune=0)
    s.update(kw)
    return [s[f] for f in KERNEL_SHAPE_FIELDS]


def ask(fn, shapes):
    """one int per row of `shapes` from a choice function of the test API (qt_wave_cascade_once and its kin)"""
    shapes = np.ascontiguousarray(shapes, dtype=np.int32)
    out = np.zeros(len(shapes), dtype=np.int32)
    fn(shapes.ctypes.data, len(shapes), out.ctypes.data)
    return [int(x) for x in out]


# ------------------------------------------------------------------------------------------------------------------ the build's resource tables
def _load_kernel_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


kernel_resources = _load_kernel_resources()


def resource_rows(units=None):
    """the rows tools/kernel_resources.py reads from csrc/build/<unit>.res, of the named units or of all"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])          # a no-op when the library is built (build() ran)
    return kernel_resources.all_rows(units)


def static_lds(unit):
    """the static LDS bytes per block of every kernel in csrc/build/<unit>.res, in the file's order"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    text = open(os.path.join(CSRC, "build", unit + ".res"), errors="replace").read()
    return [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)]


# ------------------------------------------------------------------------------------------------------------------ the sanitizer self-tests
def run_selftest(make_target, binary):
    """build a stand-alone self-test (its own main, -fsanitize=address,undefined) and run it as a child process: exit 0 and `selftest OK`"""
    subprocess.check_call(["make", "-C", CSRC, "-s", make_target])
    run = subprocess.run([os.path.join(CSRC, "build", binary)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "selftest OK" in run.stdout
    return run
