"""The tiled sweep's kernel in the build's resource tables (csrc/build/class_sweep_tiled.res): one kernel, no scratch, no static LDS -- its LDS is
the dynamic window of one tile, sweep::lds_carve(tile_width), 64 KiB at most -- and its name outside the sealed registry of ladder / wave / colour
kernels.  The reduce kernel it shares is class_sweep_cut's (tests/test_class_sweep_cut_resources.py).

VGPR budget: the build gives 12; the segment, the ops, the representative, the held words and the weights are scalar, a lane holds a local index,
its offset in the state vector and an entry.  32 keeps the full 8 waves per SIMD -- 1 024 threads need no more than 64 -- and still catches a lane
that starts to carry the plan."""
import kernel_cases
import test_class_sweep_tiled_cpu as ST
from hostlib import SEALED_HEADS, resource_rows, static_lds

KERNELS = ["k_class_sweep_tiled"]


def _rows():
    return resource_rows(["class_sweep_tiled"])


def test_one_kernel_without_scratch_that_allows_1024_threads():
    rows = _rows()
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 32 and r["Occupancy"] == 8, r


def test_no_static_lds_and_the_dynamic_window_of_one_tile():
    static = static_lds("class_sweep_tiled")
    assert static == [0], static
    T = ST.load_twin()
    for code, L, hw, tw in ST.ACCEPTED:
        rc, inf, _ = ST.info(T, code, L, hw, tw)
        assert rc == 0 and 4 <= inf["tile_width"] <= 13 and (8 << inf["tile_width"]) <= 64 * 1024 and inf["threads"] <= 1024, (code, L, hw, tw, inf)
    assert max(ST.info(T, c, L, hw, tw)[1]["tile_width"] for c, L, hw, tw in ST.ACCEPTED) == 13      # (the 64 KiB tile is among them)


def test_the_tiled_kernel_stays_out_of_the_sealed_registry():
    for r in _rows():
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()
