"""The tiled (min, +) kernels in the build's resource tables (csrc/build/class_minplus_tiled.res): exactly two kernels -- the uniform one and the one
under a cost word per qubit; the reduce stays in class_minplus's unit --, no scratch, no static LDS (their LDS is the dynamic window of one tile,
sweep::lds_carve(tile_width), 64 KiB at most), within the VGPR budget and at the occupancy tests/test_class_sweep_tiled_resources.py allows the
tiled sum-product kernel -- 32 VGPRs keep the full 8 waves per SIMD and still catch a lane that starts to carry the plan --, and their names outside
the sealed registry of ladder / wave / colour kernels.  Then the stand-alone selftest of the twins under AddressSanitizer + UBSan."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows, run_selftest, static_lds

KERNELS = ["k_class_minplus_tiled", "k_class_minplus_tiled_site"]


def test_two_kernels_without_scratch_within_the_tiled_sweeps_budget():
    rows = resource_rows(["class_minplus_tiled"])
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    theirs = {r["label"]: r for r in resource_rows(["class_sweep_tiled"])}["k_class_sweep_tiled"]
    for r in rows:
        print(r["label"], "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"], "| k_class_sweep_tiled VGPRs", theirs["VGPRs"], "occupancy", theirs["Occupancy"])
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 32 and r["Occupancy"] == 8 == theirs["Occupancy"], r


def test_no_static_lds():
    static = static_lds("class_minplus_tiled")
    assert static == [0, 0], static


def test_the_tiled_minplus_kernels_stay_out_of_the_sealed_registry():
    for r in resource_rows(["class_minplus_tiled"]):
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()


def test_the_sibling_units_keep_their_kernels():
    assert sorted(r["label"] for r in resource_rows(["class_minplus"])) == ["k_class_minplus", "k_class_minplus_reduce"]
    assert sorted(r["label"] for r in resource_rows(["class_minplus_site"])) == ["k_class_minplus_site", "k_minplus_trace_site"]
    assert sorted(r["label"] for r in resource_rows(["class_sweep_tiled"])) == ["k_class_sweep_tiled"]


def test_minplus_tiled_under_sanitizers():
    """a stand-alone program (its own main) built from class_minplus_tiled.hpp with -fsanitize=address,undefined: the tiled plans behind this entry
    point's prefixes, the twins over scratch, tables and outputs allocated at their exact size against the cut twin and a brute force, the cost-range
    checks; run as a child process"""
    run_selftest("minplus_tiled_asan", "class_minplus_tiled_selftest_asan")
