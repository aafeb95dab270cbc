"""The registry of tests/kernel_cases.py on the CPU: "built" implies "has a parity case", and every case is aimed at the kernel it claims.

  (a) completeness: the registry's labels are exactly the ladder / wave / colour / statistics / shortest-chain kernels of the build (csrc/build/*.res) --
      a kernel added to an instantiation unit without a case fails here, and so does a case whose kernel is no longer built;
  (b) pre-flight: for every case the kernel is predicted on the host -- plan_host() on the case's real parameter block, the launch mode its entry point
      presents, choose_kernel() -- and equals the case's label, before any GPU time is spent;
  the rules the cases were chosen by, as far as a row shows them.

  (c) non-vacuity -- conditions on the oracle's run alone -- is asserted in tests/test_gpu_kernel_cases.py, where the oracle half is computed anyway
      (here it would add the oracle half of every case to the suite without a GPU); `python tests/kernel_cases.py --oracle` runs it without a GPU."""
import ctypes as C

import pytest

import kernel_cases as KC

CASES = KC.load_cases()


@pytest.fixture(scope="module")
def T():
    return KC.tables_lib()


def test_every_built_kernel_has_a_case_and_every_case_a_built_kernel():
    built, have = set(KC.built_labels()), {c["label"] for c in CASES}
    assert len(built) > 300
    assert not sorted(built - have), "built kernels without a parity case (add a row to tests/kernel_cases.json): %r" % sorted(built - have)
    assert not sorted(have - built), "cases for kernels that are not built (remove the row): %r" % sorted(have - built)


def test_key_label_speaks_the_vocabulary_of_the_build():
    """kernel_resources.key_label (what qecmc._lib.last_kernel() returns) on keys written out by hand, one per family"""
    kl = KC.kernel_resources.key_label
    assert kl([1, 512, 8, 0, 2 | 256 | 1024, 0, 0, 0, 0, 0]) == "ladder<512,8,toric: gsplit|delut|ssw>"
    assert kl([1, 512, 8, 3, 0, 0, 0, 0, 0, 0]) == "ladder<512,8,planar: plain>"
    assert kl([2, 1024, 8, 1, 0, 8, 1, 0, 0, 0]) == "wave<1024,8,xzzx: 8 words, conv, queue>"
    assert kl([2, 512, 6, 2, 0, 4, 1, 10, 1, 0]) == "wave<512,6,rotated: 4 words, conv, queue, alpha, iters 10>"
    assert kl([3, 1024, 4, 2, 0, 0, 1, 0, 0, 2]) == "colour<1024,4,rotated: rule 2, conv>"
    assert kl([2, 1024, 4, 0, 1, 12, 0, 0, 0, 0]) == "wave-stats<1024,4,toric: 12 words>"
    assert kl([3, 1024, 4, 1, 1, 0, 0, 0, 0, 1]) == "colour-stats<1024,4,xzzx: rule 1>"
    assert kl([2, 1024, 4, 1, 2, 8, 1, 10, 1, 0]) == "wave-shortest<1024,4,xzzx: 8 words, iters 10>"
    assert kl([3, 1024, 4, 2, 2, 0, 1, 0, 0, 2]) == "colour-shortest<1024,4,rotated>"
    with pytest.raises(ValueError):
        kl([0] * 10)


def test_last_kernel_before_any_launch_is_an_error():
    """qecmc_last_kernel on a thread that has launched nothing: QECMC_ERR_INVALID, and a NULL buffer too (nothing here launches: no GPU needed)"""
    import threading
    from qecmc import _lib as L_
    out = {}

    def ask():
        key = (C.c_int64 * 10)()
        out["rc"] = L_.lib().qecmc_last_kernel(key)
        out["msg"] = L_.lib().qecmc_last_error()
        out["null"] = L_.lib().qecmc_last_kernel(None)
    t = threading.Thread(target=ask)
    t.start(); t.join()
    assert out["rc"] == -1 and b"launched no ladder kernel" in out["msg"] and out["null"] == -1


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_the_case_is_aimed_at_its_kernel(T, case):
    assert KC.predict(T, case) == case["label"]


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_the_case_follows_the_rules(case):
    lab = case["label"]
    assert case["entry"] in KC.ENTRIES and case["L"] >= 3 and case["first_syndrome"] > 0 and case["first_syndrome"] % 64 == 0
    assert case["iters"] == 10 if "iters 10" in lab else case["iters"] in (5, 7, 10)
    if lab.startswith("wave") and "iters 10" not in lab and "stats" not in lab:
        assert case["iters"] == 7                                    # the general-loop twins
    if lab.startswith("colour"):
        assert case["N"] == 5                                        # a workgroup per ladder
    elif "queue" in lab:
        # one workgroup of 64 lanes, every lane refilled at least twice
        assert case["queue_grid"] == 1 and case["N"] >= 200 and case["conv"] and not case["states"]
    elif case["entry"] == "ptdc":
        assert case["N"] * (16 if case["code"] == "toric" else 4) in (72, 80)      # ladders: two workgroups, the second ragged
    else:
        assert case["N"] == 70                                       # two workgroups, the second ragged
    if "<1024" in lab and "stats" not in lab and "shortest" not in lab and not lab.startswith("colour") and "uset" not in lab:
        assert case["Nc"] >= 9
    if case["entry"] != "ptdc":
        assert case["p_logical"] == 0.5                              # (the oracle's batch functions run the reference's 0.5; ptdc: no logical moves)
    if not case["conv"] and case["entry"] in ("pteq", "pteq_stats"):
        assert case["states"]                                        # fixed-length runs compare the final state of every rung
