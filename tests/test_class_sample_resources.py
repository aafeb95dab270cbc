"""The sampler's kernels in the build's resource tables: csrc/class_sample.hip is a unit of its own, so csrc/build/class_sample.res holds exactly its four
kernels -- pick, record, record_site, walk --, no scratch, no static LDS (the record kernels' LDS is the dynamic window sweep::lds_carve() promises the
launch, as k_class_sweep_cut's; the walk keeps its chain in statically indexed registers), their names outside the sealed registry of ladder / wave /
colour kernels; capi.hip, the C-ABI host file, holds no kernel; the sum-product units the sampler launches through still hold their kernels, unchanged
in number: the split of their launch functions added host functions only; and the twin's stand-alone self-test under AddressSanitizer + UBSan.  Read
the way tests/test_class_minplus_trace_resources.py reads its unit."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows, run_selftest, static_lds

UNIT = "class_sample"
KERNELS = ["k_class_sample_pick", "k_class_sample_record", "k_class_sample_record_site", "k_class_sample_walk"]


def test_sanitizers_class_sample():
    run_selftest("sample_asan", "class_sample_selftest_asan")


def test_four_kernels_without_scratch():
    rows = resource_rows([UNIT])
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        print(r["label"], "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"])
        assert r["ScratchSize"] == 0, r
        assert r["VGPRs"] <= 64, r                                               # (DESIGN.md 4.1s has the counts: 20, 13, 13 and 37)


def test_no_static_lds():
    static = static_lds(UNIT)
    assert static == [0, 0, 0, 0], static


def test_the_host_file_holds_no_kernel():
    assert resource_rows(["capi"]) == [] and static_lds("capi") == []


def test_the_sample_kernels_stay_out_of_the_sealed_registry():
    rows = resource_rows([UNIT])
    assert len(rows) == len(KERNELS)
    for r in rows:
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()


def test_the_sum_product_units_keep_their_kernels():
    cut = resource_rows(["class_sweep_cut"])
    assert sorted(r["label"] for r in cut) == ["k_class_sweep_cut", "k_class_sweep_reduce"], cut
    site = resource_rows(["class_sweep_site"])
    assert sorted(r["label"] for r in site) == ["k_class_sweep_cut_site", "k_class_sweep_site", "k_class_sweep_tiled_site"], site
    assert all(r["ScratchSize"] == 0 for r in cut + site)
