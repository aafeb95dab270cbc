"""The tiled traceback's kernels in the build's resource tables.  csrc/class_minplus_tiled_trace.hip is a unit of its own: exactly three kernels -- the two
trace kernels, no scratch, no static LDS (their LDS is the dynamic window of one tile, 64 KiB at most), within the 32 VGPRs that keep the tiled sweeps'
full 8 waves per SIMD, and the walk, one wave per pair, within 64 --, their names outside the sealed registry of ladder / wave / colour kernels;
ladder_colour_shortest.hip holds exactly its two sealed kernels, as they were built before the traceback.  Then the stand-alone selftest of the plan,
the twins and the device layout under AddressSanitizer + UBSan."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows, run_selftest, static_lds

UNIT, COLOUR = "class_minplus_tiled_trace", "ladder_colour_shortest"
TRACE, WALK = ["k_class_minplus_tiled_trace", "k_class_minplus_tiled_trace_site"], "k_minplus_tiled_walk"
SEALED = {"colour-shortest<1024,4,rotated>": (110, 4), "colour-shortest<1024,4,xzzx>": (110, 4)}         # label: (VGPRs, occupancy), profiles/r08_shortest_kernel_rows.txt


def rows():
    return {r["label"]: r for r in resource_rows([UNIT])}


def test_three_kernels_without_scratch_within_the_tiled_sweeps_budget():
    got = rows()
    assert sorted(got) == sorted(TRACE + [WALK]), sorted(got)
    theirs = {r["label"]: r for r in resource_rows(["class_minplus_tiled"])}["k_class_minplus_tiled"]
    for lab in TRACE:
        r = got[lab]
        print(lab, "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"], "| k_class_minplus_tiled VGPRs", theirs["VGPRs"], "occupancy", theirs["Occupancy"])
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 32 and r["Occupancy"] == 8 == theirs["Occupancy"], r
    r = got[WALK]
    print(WALK, "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"])
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] == 8, r


def test_no_static_lds():
    static = static_lds(UNIT)
    assert static == [0] * 3, static
    assert static_lds(COLOUR) == [0, 0]


def test_the_traceback_kernels_stay_out_of_the_sealed_registry():
    for lab in TRACE + [WALK]:
        assert not lab.startswith(SEALED_HEADS) and lab not in kernel_cases.built_labels()


def test_the_host_units_sealed_kernels_are_unchanged():
    got = {r["label"]: r for r in resource_rows([COLOUR])}
    assert set(got) == set(SEALED)
    for lab, (vgprs, occupancy) in SEALED.items():
        assert (got[lab]["VGPRs"], got[lab]["Occupancy"], got[lab]["ScratchSize"]) == (vgprs, occupancy, 0), got[lab]
    # ... and the shipped sweep units keep their kernels: the traceback adds none to them
    assert sorted(r["label"] for r in resource_rows(["class_minplus_tiled"])) == ["k_class_minplus_tiled", "k_class_minplus_tiled_site"]
    assert sorted(r["label"] for r in resource_rows(["class_minplus_trace"])) == ["k_minplus_pick", "k_minplus_trace", "k_minplus_walk"]


def test_minplus_tiled_trace_under_sanitizers():
    """a stand-alone program (its own main) built from class_minplus_tiled_trace.hpp with -fsanitize=address,undefined: the trace plans and their refusals,
    the twins over poisoned buffers of exact size against the cut twin, and a host walk of the device layout -- tile by tile through the segment table,
    forget_tile addressing, a dirty decision block -- that gives the twin's chains byte for byte; run as a child process"""
    run_selftest("minplus_tiled_trace_asan", "class_minplus_tiled_trace_selftest_asan")
