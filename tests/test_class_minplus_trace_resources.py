"""The traceback's kernels in the build's resource tables (csrc/build/class_minplus_trace.res): three kernels -- pick, trace, walk --, no scratch, no
static LDS (the trace kernel's LDS is the dynamic window sweep::lds_carve() promises the launch, as k_class_minplus's; pick and walk reduce and
unpack through shuffles and have none), their names outside the sealed registry of ladder / wave / colour kernels; and class_minplus.res still holds
its two kernels: the split of launch_class_minplus added host functions only.  Read the way tests/test_class_minplus_resources.py reads its unit."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows, static_lds
from test_class_minplus_resources import KERNELS as MINPLUS_KERNELS

KERNELS = ["k_minplus_pick", "k_minplus_trace", "k_minplus_walk"]


def test_three_kernels_without_scratch():
    rows = resource_rows(["class_minplus_trace"])
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        print(r["label"], "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"])
        assert r["ScratchSize"] == 0, r


def test_no_static_lds():
    static = static_lds("class_minplus_trace")
    assert static == [0, 0, 0], static


def test_the_trace_kernels_stay_out_of_the_sealed_registry():
    for r in resource_rows(["class_minplus_trace"]):
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()


def test_class_minplus_keeps_its_two_kernels():
    rows = resource_rows(["class_minplus"])
    assert sorted(r["label"] for r in rows) == MINPLUS_KERNELS == ["k_class_minplus", "k_class_minplus_reduce"], rows
    assert all(r["ScratchSize"] == 0 for r in rows)
