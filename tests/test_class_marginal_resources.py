"""The marginals' kernels in the build's resource tables: csrc/class_marginal.hip is a unit of its own, so csrc/build/class_marginal.res holds exactly
its six kernels -- fwd, fwd_site, bwd, bwd_site, fold, combine --, without scratch and without static LDS (the forward and backward kernels' LDS is the
dynamic window sweep::lds_carve() promises the launch, as k_class_sweep_cut's), their names outside the sealed registry of ladder / wave / colour
kernels; primitives.hip holds exactly its nine byte-state kernels, capi.hip none, and the pinned units still exactly theirs; and the twin's
stand-alone self-test under AddressSanitizer + UBSan.  Read the way tests/test_class_sample_resources.py reads its unit."""
import kernel_cases
from hostlib import SEALED_HEADS, resource_rows, run_selftest, static_lds

UNIT = "class_marginal"
KERNELS = ["k_class_marginal_bwd", "k_class_marginal_bwd_site", "k_class_marginal_combine", "k_class_marginal_fold", "k_class_marginal_fwd", "k_class_marginal_fwd_site"]
PRIMITIVES = ["k_apply_logical", "k_apply_stabilizer", "k_chain_update", "k_count_errors", "k_eq_class", "k_generate_errors", "k_hide_class", "k_syndrome", "k_to_class"]


def test_sanitizers_class_marginal():
    run_selftest("marginal_asan", "class_marginal_selftest_asan")


def test_six_kernels_without_scratch():
    rows = resource_rows([UNIT])
    assert sorted(r["label"] for r in rows) == KERNELS, rows
    for r in rows:
        print(r["label"], "VGPRs", r["VGPRs"], "occupancy", r["Occupancy"])
        assert r["ScratchSize"] == 0, r
        assert r["VGPRs"] <= 64, r                                               # (DESIGN.md 4.1t has the counts)


def test_no_static_lds():
    static = static_lds(UNIT)
    assert static == [0] * len(KERNELS), static


def test_the_marginal_kernels_stay_out_of_the_sealed_registry():
    rows = resource_rows([UNIT])
    assert len(rows) == len(KERNELS)
    for r in rows:
        assert not r["label"].startswith(SEALED_HEADS)
        assert r["label"] not in kernel_cases.built_labels()


def test_the_unit_keeps_its_kernels_and_the_pinned_units_theirs():
    assert sorted(r["label"] for r in resource_rows(["primitives"])) == PRIMITIVES
    cut = resource_rows(["class_sweep_cut"])
    assert sorted(r["label"] for r in cut) == ["k_class_sweep_cut", "k_class_sweep_reduce"], cut
    assert resource_rows(["capi"]) == []
    sample = resource_rows(["class_sample"])
    assert sorted(r["label"] for r in sample) == ["k_class_sample_pick", "k_class_sample_record", "k_class_sample_record_site", "k_class_sample_walk"], sample
