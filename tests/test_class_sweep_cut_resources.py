"""The cut-set sweep's kernels in the build's resource tables (csrc/build/class_sweep_cut.res): two kernels, no scratch, no static LDS -- the sweep
kernel's LDS is the dynamic window sweep::lds_carve() promises the launch, up to 128 KiB at width 14; the reduce kernel has none -- and their names
outside the sealed registry of ladder / wave / colour kernels.

VGPR budget: the build gives 11 (sweep) and 12 (reduce); the plan, the representative, the held words and the weights are scalar, a lane holds an
index and an entry.  32 keeps the full 8 waves per SIMD with room to spare and still catches a lane that starts to carry the plan."""
import kernel_cases
import test_class_sweep_cut_cpu as SC
from hostlib import SEALED_HEADS, resource_rows, static_lds

KERNELS = ["k_class_sweep_cut", "k_class_sweep_reduce"]


def _rows():
    return resource_rows(["class_sweep_cut"])


def test_two_kernels_without_scratch():
    rows = _rows()
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 32 and r["Occupancy"] == 8, r


def test_no_static_lds_and_the_dynamic_window_the_host_function_sizes():
    static = static_lds("class_sweep_cut")
    assert static == [0, 0], static
    T = SC.load_twin()
    for code, L, w in SC.ACCEPTED:
        rc, inf, _ = SC.info(T, code, L, w)
        assert rc == 0 and 0 < inf["lds_bytes"] == 8 << inf["width"] <= 128 * 1024, (code, L, w, inf)
    assert max(SC.info(T, c, L, w)[1]["lds_bytes"] for c, L, w in SC.ACCEPTED) == 128 * 1024        # (the 128 KiB path is among them)


def test_the_cut_kernels_stay_out_of_the_sealed_registry():
    for r in _rows():
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()
