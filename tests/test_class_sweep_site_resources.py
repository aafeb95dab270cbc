"""The site sweeps' kernels in the build's resource tables (csrc/build/class_sweep_site.res): exactly the three new kernels, no scratch, no static LDS
-- their LDS is the dynamic window their siblings ask for -- and their names outside the sealed registry of ladder / wave / colour kernels.  The
reduce kernel the cut and the tiled route share is class_sweep_cut's (tests/test_class_sweep_cut_resources.py); the old units keep their own lists.

VGPR budget: the build gives 11 or 12; the plan, the representative, the held words AND the four weights of a CLOSE are scalar -- the table's row is
wave-uniform --, a lane holds an index and an entry.  32 keeps the full 8 waves per SIMD under 1 024 threads and catches a lane that starts to carry
the table."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows, static_lds

KERNELS = ["k_class_sweep_cut_site", "k_class_sweep_site", "k_class_sweep_tiled_site"]


def _rows():
    return resource_rows(["class_sweep_site"])


def test_three_kernels_without_scratch_at_full_occupancy():
    rows = _rows()
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 32 and r["Occupancy"] == 8, r


def test_no_static_lds():
    static = static_lds("class_sweep_site")
    assert static == [0, 0, 0], static                                 # all of it is asked for at the launch, as the siblings ask


def test_the_site_kernels_stay_out_of_the_sealed_registry():
    for r in _rows():
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()
