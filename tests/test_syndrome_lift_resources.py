"""The syndrome-lift kernel in the build's resource tables (csrc/build/syndrome_lift.res): no scratch -- its per-lane state lives in LDS, not in
a dynamically indexed register array -- and a name of its own, outside the sealed registry of ladder / wave / colour kernels that
tests/kernel_cases.json enumerates."""
from hostlib import SEALED_HEADS, resource_rows


def test_lift_kernel_uses_no_scratch_and_stays_out_of_the_sealed_registry():
    rows = resource_rows(["syndrome_lift"])
    assert [r["label"] for r in rows] == ["k_syndrome_lift"], rows
    for r in rows:
        assert r["ScratchSize"] == 0, r
        assert not r["label"].startswith(SEALED_HEADS), r
        assert r["VGPRs"] <= 64, r                                     # (8 waves per SIMD: the launch is one wave per workgroup, many per CU)
