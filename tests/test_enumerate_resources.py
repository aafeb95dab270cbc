"""The coset-enumeration kernels in the build's resource tables (csrc/build/enumerate.res): both instantiations are built (4 and 16 classes), neither
uses scratch, their LDS is the dynamic window alone -- no static LDS on top of what enumr::lds_carve() promises the launch, which stays within
64 KiB for every supported shape -- and their name stays outside the sealed registry of ladder / wave / colour kernels."""
import re

import kernel_cases
import test_enumerate_cpu as E
from hostlib import SEALED_HEADS, resource_rows, static_lds


def _rows():
    return resource_rows(["enumerate"])


def test_both_instantiations_are_built_without_scratch():
    rows = _rows()
    assert [r["label"] for r in rows] == ["k_enumerate", "k_enumerate"], rows
    assert sorted(re.search(r"k_enumerateILi(\d+)ELi(\d+)E", r["kernel"]).groups() for r in rows) == [("16", "4"), ("4", "6")]    # <NCLS, T>
    for r in rows:
        assert r["ScratchSize"] == 0, r
        assert r["VGPRs"] <= 64, r                                     # (the unrolled walk keeps its generators and representatives in scalar registers)


def test_lds_is_the_dynamic_window_the_host_function_sizes():
    static = static_lds("enumerate")
    assert static == [0, 0], static                                    # all of it is asked for at the launch: enumr::lds_carve()
    T = E.load_twin()
    for code, L in E.SUPPORTED:
        rc, inf, _ = E.info(T, code, L)
        assert rc == 0 and 0 < inf["lds_bytes"] <= 64 * 1024, (code, L, inf)


def test_enumerate_kernels_stay_out_of_the_sealed_registry():
    label = _rows()[0]["label"]
    assert not label.startswith(SEALED_HEADS)
    assert label not in kernel_cases.built_labels()
