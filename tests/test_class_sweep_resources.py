"""The frontier-sweep kernel in the build's resource tables (csrc/build/class_sweep.res): one kernel, no scratch, its LDS the dynamic window alone -- no
static LDS on top of what sweep::lds_carve() promises the launch, which stays within 64 KiB for every accepted plan -- and its name outside the sealed
registry of ladder / wave / colour kernels."""
import importlib.util
import os
import re
import subprocess

import kernel_cases
import test_class_sweep_cpu as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc")
SEALED_HEADS = ("ladder<", "wave<", "colour<", "wave-stats<", "colour-stats<", "wave-shortest<", "colour-shortest<")


def _rows():
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])          # a no-op when the library is built (build() ran)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.all_rows(["class_sweep"])


def test_one_kernel_without_scratch():
    rows = _rows()
    assert [r["label"] for r in rows] == ["k_class_sweep"], rows
    assert rows[0]["ScratchSize"] == 0, rows
    assert rows[0]["VGPRs"] <= 64, rows                                # (the plan, the representative and the weights are scalar: a lane holds an index and an entry)


def test_lds_is_the_dynamic_window_the_host_function_sizes():
    _rows()
    text = open(os.path.join(CSRC, "build", "class_sweep.res"), errors="replace").read()
    static = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)]
    assert static == [0], static                                       # all of it is asked for at the launch: sweep::lds_carve()
    T = S.load_twin()
    for code, L in S.REQUIRED:
        rc, inf, _ = S.info(T, code, L)
        assert rc == 0 and 0 < inf["lds_bytes"] == 8 << inf["width"] <= 64 * 1024, (code, L, inf)


def test_the_sweep_kernel_stays_out_of_the_sealed_registry():
    label = _rows()[0]["label"]
    assert not label.startswith(SEALED_HEADS)
    assert label not in kernel_cases.built_labels()
