"""The (min, +, count) sweep's kernels in the build's resource tables (csrc/build/class_minplus.res): two kernels, no scratch, no static LDS -- the
sweep kernel's LDS is the dynamic window sweep::lds_carve() promises the launch, one uint64_t where the sibling keeps a double, up to 128 KiB at
width 14; the reduce kernel has none -- and their names outside the sealed registry of ladder / wave / colour kernels.  Read the way
tests/test_class_sweep_cut_resources.py reads its siblings.  The VGPR counts are recorded in DESIGN.md 4.1o, not bounded here."""
import kernel_cases
import test_class_sweep_cut_cpu as SC
from hostlib import SEALED_HEADS, resource_rows, static_lds

KERNELS = ["k_class_minplus", "k_class_minplus_reduce"]


def _rows():
    return resource_rows(["class_minplus"])


def test_two_kernels_without_scratch():
    rows = _rows()
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        print(r["label"], "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"])
        assert r["ScratchSize"] == 0, r


def test_no_static_lds_and_the_dynamic_window_the_host_function_sizes():
    static = static_lds("class_minplus")
    assert static == [0, 0], static
    T = SC.load_twin()
    for code, L, w in SC.ACCEPTED:                                     # the plans are the cut sweep's: a uint64_t entry is as wide as its double
        rc, inf, _ = SC.info(T, code, L, w)
        assert rc == 0 and 0 < inf["lds_bytes"] == 8 << inf["width"] <= 128 * 1024, (code, L, w, inf)


def test_the_minplus_kernels_stay_out_of_the_sealed_registry():
    for r in _rows():
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()
