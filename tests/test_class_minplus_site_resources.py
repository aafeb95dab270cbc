"""The site-cost kernels in the build's resource tables (csrc/build/class_minplus_site.res): exactly two kernels -- the sweep and the trace under a
cost word per qubit; the reduce, the pick and the walk stay in the siblings' units --, no scratch, no static LDS (their LDS is the dynamic window
sweep::lds_carve() promises the launch), a compiler-reported occupancy not below the uniform sibling's of the same build, and their names outside the
sealed registry of ladder / wave / colour kernels.  Read the way tests/test_class_minplus_trace_resources.py reads its unit."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows, static_lds
from test_class_minplus_trace_resources import KERNELS as TRACE_KERNELS

KERNELS = ["k_class_minplus_site", "k_minplus_trace_site"]
SIBLING = {"k_class_minplus_site": ("class_minplus", "k_class_minplus"), "k_minplus_trace_site": ("class_minplus_trace", "k_minplus_trace")}


def test_two_kernels_without_scratch():
    rows = resource_rows(["class_minplus_site"])
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        print(r["label"], "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"])
        assert r["ScratchSize"] == 0, r


def test_no_static_lds():
    static = static_lds("class_minplus_site")
    assert static == [0, 0], static


def test_occupancy_is_not_below_the_uniform_siblings():
    mine = {r["label"]: r for r in resource_rows(["class_minplus_site"])}
    for label, (unit, sibling) in SIBLING.items():
        theirs = {r["label"]: r for r in resource_rows([unit])}[sibling]
        print(label, "occupancy", mine[label]["Occupancy"], "VGPRs", mine[label]["VGPRs"], "|", sibling, "occupancy", theirs["Occupancy"], "VGPRs", theirs["VGPRs"])
        assert mine[label]["Occupancy"] >= theirs["Occupancy"] > 0, (mine[label], theirs)


def test_the_site_kernels_stay_out_of_the_sealed_registry():
    for r in resource_rows(["class_minplus_site"]):
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()


def test_the_uniform_units_keep_their_kernels():
    assert sorted(r["label"] for r in resource_rows(["class_minplus"])) == ["k_class_minplus", "k_class_minplus_reduce"]
    assert sorted(r["label"] for r in resource_rows(["class_minplus_trace"])) == TRACE_KERNELS
