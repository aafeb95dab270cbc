"""The frontier-sweep kernel in the build's resource tables (csrc/build/class_sweep.res): one kernel, no scratch, its LDS the dynamic window alone -- no
static LDS on top of what sweep::lds_carve() promises the launch, which stays within 64 KiB for every accepted plan -- and its name outside the sealed
registry of ladder / wave / colour kernels."""
import kernel_cases
import test_class_sweep_cpu as S
from hostlib import SEALED_HEADS, resource_rows, static_lds


def _rows():
    return resource_rows(["class_sweep"])


def test_one_kernel_without_scratch():
    rows = _rows()
    assert [r["label"] for r in rows] == ["k_class_sweep"], rows
    assert rows[0]["ScratchSize"] == 0, rows
    assert rows[0]["VGPRs"] <= 64, rows                                # (the plan, the representative and the weights are scalar: a lane holds an index and an entry)


def test_lds_is_the_dynamic_window_the_host_function_sizes():
    static = static_lds("class_sweep")
    assert static == [0], static                                       # all of it is asked for at the launch: sweep::lds_carve()
    T = S.load_twin()
    for code, L in S.REQUIRED:
        rc, inf, _ = S.info(T, code, L)
        assert rc == 0 and 0 < inf["lds_bytes"] == 8 << inf["width"] <= 64 * 1024, (code, L, inf)


def test_the_sweep_kernel_stays_out_of_the_sealed_registry():
    label = _rows()[0]["label"]
    assert not label.startswith(SEALED_HEADS)
    assert label not in kernel_cases.built_labels()
