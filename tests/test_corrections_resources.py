"""The corrections kernel in the build's resource tables (csrc/build/corrections.res): no scratch -- its one per-lane state lives in LDS, the K
candidates pass through it -- at most 64 vector registers, and a name of its own, outside the sealed registry of ladder / wave / colour kernels that
tests/kernel_cases.json enumerates."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows


def _rows():
    return resource_rows(["corrections"])


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
