"""The marginals' kernels in the build's resource tables: csrc/class_marginal.inc is compiled as the tail of primitives.hip -- the set of HIP units is
pinned, and that unit is the one whose kernel list no test pins --, so csrc/build/primitives.res holds the unit's old kernels and the six new ones --
fwd, fwd_site, bwd, bwd_site, fold, combine --, these without scratch and without static LDS (the forward and backward kernels' LDS is the dynamic
window sweep::lds_carve() promises the launch, as k_class_sweep_cut's), their names outside the sealed registry of ladder / wave / colour kernels;
the pinned units still hold exactly their kernels; and the twin's stand-alone self-test under AddressSanitizer + UBSan.  Read the way
tests/test_class_sample_resources.py reads its unit."""
import os
import re

import kernel_cases
from hostlib import CSRC, SEALED_HEADS, resource_rows, run_selftest

KERNELS = ["k_class_marginal_bwd", "k_class_marginal_bwd_site", "k_class_marginal_combine", "k_class_marginal_fold", "k_class_marginal_fwd", "k_class_marginal_fwd_site"]
# what primitives.hip held before the marginals were added to its tail
BEFORE = ["k_apply_logical", "k_apply_stabilizer", "k_chain_update", "k_count_errors", "k_eq_class", "k_generate_errors", "k_hide_class", "k_syndrome", "k_to_class"]


def test_sanitizers_class_marginal():
    run_selftest("marginal_asan", "class_marginal_selftest_asan")


def new_rows():
    return [r for r in resource_rows(["primitives"]) if r["label"].startswith("k_class_marginal")]


def test_six_kernels_without_scratch():
    rows = new_rows()
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        print(r["label"], "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"])
        assert r["ScratchSize"] == 0, r
        assert r["VGPRs"] <= 64, r                                               # (DESIGN.md 4.1t has the counts)


def test_no_static_lds():
    assert resource_rows(["primitives"])                                        # (builds the unit where it is not built)
    text = open(os.path.join(CSRC, "build", "primitives.res"), errors="replace").read()
    blocks = re.findall(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", text, flags=re.S)
    mine = {name: int(lds) for name, lds in blocks if "k_class_marginal" in name}
    assert len(mine) == len(KERNELS) and set(mine.values()) == {0}, mine


def test_the_marginal_kernels_stay_out_of_the_sealed_registry():
    for r in new_rows():
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()


def test_the_unit_keeps_its_kernels_and_the_pinned_units_theirs():
    rest = sorted(r["label"] for r in resource_rows(["primitives"]) if not r["label"].startswith("k_class_marginal"))
    assert rest == BEFORE, rest
    cut = resource_rows(["class_sweep_cut"])
    assert sorted(r["label"] for r in cut) == ["k_class_sweep_cut", "k_class_sweep_reduce"], cut
    capi = resource_rows(["capi"])
    assert sorted(r["label"] for r in capi) == ["k_class_sample_pick", "k_class_sample_record", "k_class_sample_record_site", "k_class_sample_walk"], capi
