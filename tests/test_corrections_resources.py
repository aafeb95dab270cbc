"""The corrections kernel in the build's resource tables (csrc/build/corrections.res): no scratch -- its one per-lane state lives in LDS, the K
candidates pass through it -- at most 64 vector registers, and a name of its own, outside the sealed registry of ladder / wave / colour kernels that
tests/kernel_cases.json enumerates."""
import importlib.util
import os
import subprocess

import kernel_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc")
SEALED_HEADS = ("ladder<", "wave<", "colour<", "wave-stats<", "colour-stats<", "wave-shortest<", "colour-shortest<")


def _rows():
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])          # a no-op when the library is built (build() ran)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.all_rows(["corrections"])


def test_corrections_kernel_uses_no_scratch_and_at_most_64_vgprs():
    rows = _rows()
    assert [r["label"] for r in rows] == ["k_corrections"], rows
    for r in rows:
        assert r["ScratchSize"] == 0, r
        assert r["VGPRs"] <= 64, r                                     # (8 waves per SIMD: the launch is one wave per workgroup, many per CU)


def test_corrections_kernel_stays_out_of_the_sealed_registry():
    label = _rows()[0]["label"]
    assert not label.startswith(SEALED_HEADS)
    assert label not in kernel_cases.built_labels()
