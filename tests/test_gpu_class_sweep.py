"""The exact class law by a frontier sweep on the GPU (qecmc_class_sweep): the kernel's class weights equal the host twin's -- the plain loop of
csrc/class_sweep.hpp compiled by g++, which tests/test_class_sweep_cpu.py pins against the enumerator, a brute force and an independent elimination --
BIT FOR BIT: every entry of the state vector sees the same copies, multiplies and adds on both sides.  Then the sweep against the enumeration kernel
on the same chains, the all-ones pin at L = 9 on the device, recycled device blocks, and method "exact" of the harness at the shapes the library is
benchmarked at: xzzx L = 7 and rotated L = 7."""
import numpy as np
import pytest

import test_class_sweep_cpu as cpu
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors

pytestmark = pytest.mark.gpu

NAME = cpu.NAME
W4 = np.array([1.0, 0.043, 0.019, 0.21])                                        # (w_X != w_Y != w_Z: a swapped weight shows)


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return cpu.load_twin()


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([23, code, L, seed]))


def same(got, want_z, want_cls):
    assert got["Z"].dtype == np.float64 and got["Z"].shape == want_z.shape
    assert np.array_equal(got["Z"].view(np.uint64), want_z.view(np.uint64))
    assert got["cls"].dtype == np.int32 and np.array_equal(got["cls"], want_cls)


# (code, L, N): width 4 -- fewer entries than a wavefront has lanes; the planar code's unused cells; 16 classes, dependent generators and the widest
# plan (13); width 8; the benchmark shapes: width 10, and width 12 with 81 qubits in six state words; planar at width 12
@pytest.mark.parametrize("code,L,N", [(XZZX, 3, 7), (PLANAR, 3, 3), (TORIC, 3, 3), (ROTATED, 5, 4), (XZZX, 7, 5), (ROTATED, 9, 3), (PLANAR, 6, 2)])
def test_gpu_equals_host_twin_bit_for_bit(q, T, code, L, N):
    chains = chains_of(code, L, N)
    want, cls = cpu.twin(T, code, L, chains, W4)
    got = q.class_sweep(NAME[code], chains, W4)
    same(got, want, cls)
    assert got["width"] == cpu.info(T, code, L)[1]["width"] and np.all(want > 0)


def test_syndrome_groups_with_a_ragged_last_group(q, T):
    """N = 1 029: a group of 1 024 syndromes and one of 5 (sweep::kGroupMax)"""
    chains = chains_of(XZZX, 3, 1029)
    want, cls = cpu.twin(T, XZZX, 3, chains, W4)
    same(q.class_sweep("xzzx", chains, W4), want, cls)
    assert len({z.tobytes() for z in want}) > 100                               # (many different syndromes: a row in the wrong place would show)


@pytest.mark.parametrize("code", [XZZX, ROTATED])
def test_sweep_is_the_enumeration_kernel_at_L5(q, code):
    from qecmc import exact as ex
    chains = chains_of(code, 5, 3)
    hist = q.coset_enumerator(NAME[code], chains)["hist"]
    for w4, wh in zip(cpu.FAMILIES, cpu.HIST_WEIGHTS):
        z = q.class_sweep(NAME[code], chains, w4)["Z"]
        want = ex.class_weights(hist, wh)
        assert (np.abs(z - want) / want).max() < 1e-12
    for kw in (dict(p=0.12), dict(p=0.2, eta=5.0), dict(p=0.3, alpha=2.0)):
        a = q.exact_class_probabilities(NAME[code], chains, **kw)
        assert np.array_equal(a, q.exact_class_probabilities(NAME[code], chains, method="enumerate", **kw))       # auto: what it returned before
        assert np.abs(q.exact_class_probabilities(NAME[code], chains, method="sweep", **kw) - a).max() < 1e-12


def test_all_ones_weights_count_the_group_at_L9(q):
    z = q.class_sweep("rotated", chains_of(ROTATED, 9, 2), np.ones(4))["Z"]
    assert np.all(z == 2.0 ** 80)


def test_dirty_recycled_blocks_do_not_leak_into_the_next_call(q, T):
    """the device blocks of a small call come back from the pool as the last call left them, and so does the LDS of a workgroup: the same call before
    and after a call of another shape"""
    a, b = chains_of(XZZX, 5, 2, seed=1), chains_of(PLANAR, 4, 3, seed=2)
    wa, ca = cpu.twin(T, XZZX, 5, a, W4)
    wb, cb = cpu.twin(T, PLANAR, 4, b, W4)
    same(q.class_sweep("xzzx", a, W4), wa, ca)
    same(q.class_sweep("planar", b, W4), wb, cb)
    same(q.class_sweep("xzzx", a, W4), wa, ca)


# ------------------------------------------------------------------------------------------------------ method "exact" where the library is measured
def test_generate_exact_from_syndromes_with_corrections_at_L7(q):
    from qecmc import harness
    params = dict(code="xzzx", size=7, p_error=0.1, noise="depolarizing", method="exact")
    out = harness.generate(params, 256, seed=5, start="syndrome", corrections=True)
    assert "counts" not in out and out["distr"].dtype == np.float64 and out["distr"].shape == (256, 4)
    assert np.allclose(out["distr"].sum(axis=1), 1.0, atol=1e-12)
    assert np.array_equal(out["success_correction"], out["success"])
    assert 0.6 < out["success"].mean() <= 1.0


@pytest.mark.parametrize("noise,extra", [("depolarizing", {}), ("biased", dict(eta=3.0)), ("alpha", dict(alpha=2.0))])
def test_decode_syndromes_exact_is_the_twin_law_at_L7(q, T, noise, extra):
    from qecmc import exact as ex
    from qecmc import harness
    errors = chains_of(ROTATED, 7, 24)
    defects = harness.syndrome_of("rotated", errors)
    params = dict(code="rotated", size=7, p_error=0.12, noise=noise, method="exact", **extra)
    out = harness.decode_syndromes(params, defects, corrections=True, biased_decoder="alpha")
    w4 = ex.alpha_w4(0.12, 2.0) if noise == "alpha" else ex.biased_w4(0.12, 3.0) if noise == "biased" else ex.depolarizing_w4(0.12)
    z, _ = cpu.twin(T, ROTATED, 7, out["chains"], w4)
    want = z / z.sum(axis=1, keepdims=True)
    assert np.abs(out["distr"] - want).max() < 1e-12 and "counts" not in out
    assert np.array_equal(out["target"], np.argmax(want, axis=1))
    assert np.array_equal(harness.syndrome_of("rotated", out["correction"]), defects)


def test_pteq_does_not_beat_the_exact_decoder_at_L7(q):
    """paired on one batch (McNemar), as tests/test_gpu_enumerate.py does at L = 3: a = exact right and PTEQ wrong, b = the reverse.  The exact decoder
    maximises the success probability, so E[a - b] >= 0; b - a <= 5 sqrt(a + b) is 5 sigma of the paired difference.
    The test has power only where decoders can differ: on rows whose exact law leaves the runner-up class a real chance.  That is a property of the
    batch, read off the exact law alone: at least 100 of the 2 048 rows have a runner-up with probability above 0.05, and the exact decoder itself
    fails on at least 20 rows -- a decoder that picked the runner-up on those rows would move a + b by that many."""
    from qecmc import harness
    params = dict(code="xzzx", size=7, p_error=0.15, noise="depolarizing")
    n = 2048
    exact = harness.generate(dict(params, method="exact"), n, seed=11, device_generation=True)
    second = np.sort(exact["distr"], axis=1)[:, -2]
    print("rows with a runner-up above 0.05: %d, exact failures: %d" % ((second > 0.05).sum(), (~exact["success"]).sum()))
    assert (second > 0.05).sum() >= 100 and (~exact["success"]).sum() >= 20
    pteq = harness.generate(params, n, seed=11, steps=2000, conv_criteria=None, device_generation=True)
    assert np.array_equal(pteq["qubit_matrix"], exact["qubit_matrix"]) and np.array_equal(pteq["eq_true"], exact["eq_true"])
    a = int((exact["success"] & ~pteq["success"]).sum())
    b = int((~exact["success"] & pteq["success"]).sum())
    print("exact right / PTEQ wrong: %d, the reverse: %d, success exact %.4f PTEQ %.4f" % (a, b, exact["success"].mean(), pteq["success"].mean()))
    assert b - a <= 5 * np.sqrt(a + b)
