"""The tiled sampler's kernels in the build's resource tables.  csrc/class_sample_tiled.hip is a unit of its own: exactly three kernels -- the two
record kernels, no scratch, no static LDS (their LDS is the dynamic window of one tile, 64 KiB at most), at the 8 waves per SIMD k_class_sweep_tiled
of the same build runs at, and the walk, one lane per sample, within 64 VGPRs --, their names outside the sealed registry of ladder / wave / colour
kernels; the units the family reads from keep their kernels, and the unit that took the systematic-sweep dispatch keeps the sealed labels of both.
Then the stand-alone selftest of the plan, the twin and the device layout under AddressSanitizer + UBSan."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows, run_selftest, static_lds

UNIT = "class_sample_tiled"
RECORD, WALK = ["k_class_sample_tiled_record", "k_class_sample_tiled_record_site"], "k_class_sample_tiled_walk"


def rows():
    return {r["label"]: r for r in resource_rows([UNIT])}


def test_three_kernels_without_scratch_at_the_tiled_sweeps_occupancy():
    got = rows()
    assert sorted(got) == sorted(RECORD + [WALK]), sorted(got)
    theirs = {r["label"]: r for r in resource_rows(["class_sweep_tiled"])}["k_class_sweep_tiled"]
    for lab in RECORD:
        r = got[lab]
        print(lab, "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"], "| k_class_sweep_tiled VGPRs", theirs["VGPRs"], "occupancy", theirs["Occupancy"])
        assert r["ScratchSize"] == 0 and r["Occupancy"] == 8 == theirs["Occupancy"], r
    r = got[WALK]
    print(WALK, "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"])
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64, r


def test_no_static_lds():
    static = static_lds(UNIT)
    assert static == [0] * 3, static


def test_the_sampler_kernels_stay_out_of_the_sealed_registry():
    built = sorted(rows())                                                      # the labels the build left in class_sample_tiled.res
    assert len(built) == 3
    for lab in built:
        assert lab.startswith("k_class_sample_tiled_") and not lab.startswith(SEALED_HEADS) and lab not in kernel_cases.built_labels()


def test_the_units_around_it_keep_their_kernels():
    assert sorted(r["label"] for r in resource_rows(["class_sweep_tiled"])) == ["k_class_sweep_tiled"]
    assert sorted(r["label"] for r in resource_rows(["class_sample"])) == ["k_class_sample_pick", "k_class_sample_record", "k_class_sample_record_site", "k_class_sample_walk"]
    assert sorted(r["label"] for r in resource_rows(["class_minplus_tiled_trace"])) == ["k_class_minplus_tiled_trace", "k_class_minplus_tiled_trace_site",
                                                                                       "k_minplus_tiled_walk"]
    # the systematic sweep's dispatch lives in ladder_uset.hip: that unit holds sealed ladder kernels alone, every one a label the registry builds
    uset = [r["label"] for r in resource_rows(["ladder_uset"])]
    assert uset and all(lab.startswith("ladder<") for lab in uset)
    assert any("scan" in lab for lab in uset) and any("uset" in lab for lab in uset)


def test_sample_tiled_under_sanitizers():
    """a stand-alone program (its own main) built from class_sample_tiled.hpp with -fsanitize=address,undefined: the sample plans, their refusals and the
    record cap, the twin over poisoned buffers of exact size in both modes, and a host walk of the device layout -- tile by tile through the segment
    table, pairs into a dirty block of exactly bytes_per_job bytes, read back through forget_tile -- that gives the twin's chains byte for byte; run as
    a child process"""
    run_selftest("sample_tiled_asan", "class_sample_tiled_selftest_asan")
