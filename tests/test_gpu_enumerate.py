"""The exact class law by coset enumeration on the GPU (qecmc_coset_enumerate): the kernel's histogram equals the host twin's -- the plain loop of
csrc/enumerate.hpp compiled by g++, which tests/test_enumerate_cpu.py pins against independent enumerations -- exactly, at the smallest shapes that
can go wrong; method "exact" of the harness composes with the lift and the corrections; the exact decoder is not beaten by PTEQ on one batch; and
the planar sampler is pinned on an exact law for the first time.

The xzzx / rotated codes exist at odd L only (tests/test_enumerate_cpu.py), so what an even L would exercise runs on valid shapes: many launches
per syndrome at toric L = 3 with chunk_bits = 10 (64 of them), the syndrome-group loop with a ragged last group at xzzx L = 3 with N = 1 029
(groups of 1 024), the high basis bits at L = 5."""
import numpy as np
import pytest

import test_enumerate_cpu as cpu
from test_exact_cpu import _enum, _rand_surf
from test_syndrome_lift_cpu import ORC_CODE, PLANAR, ROTATED, TORIC, XZZX, random_errors

pytestmark = pytest.mark.gpu

NAME = {TORIC: "toric", XZZX: "xzzx", ROTATED: "rotated", PLANAR: "planar"}


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return cpu.load_twin()


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([21, code, L, seed]))


def same(got, want_hist, want_cls, rank):
    assert got["hist"].dtype == np.uint64 and got["hist"].shape == want_hist.shape
    assert np.array_equal(got["hist"], want_hist)
    assert got["cls"].dtype == np.int32 and np.array_equal(got["cls"], want_cls)
    assert got["rank"] == rank


# (code, L, N, chunk_bits): rank 8 -- fewer elements than one workgroup has threads; 16 classes; the planar code's unused cells, and nq = 32 filling the
# plane; 64 launches per syndrome; two launches per syndrome in workgroups of one pass
@pytest.mark.parametrize("code,L,N,chunk_bits", [(XZZX, 3, 7, 0), (ROTATED, 3, 7, 0), (TORIC, 3, 3, 0), (PLANAR, 3, 3, 0), (PLANAR, 4, 2, 0), (TORIC, 3, 5, 10),
                                                 (PLANAR, 3, 5, 11)])
def test_gpu_equals_host_twin(q, T, code, L, N, chunk_bits):
    chains = chains_of(code, L, N)
    want, cls = cpu.twin(T, code, L, chains, chunk_bits)
    got = q.coset_enumerator(NAME[code], chains, chunk_bits=chunk_bits)
    same(got, want, cls, cpu.RANK[code, L])
    assert np.all(got["hist"].sum(axis=(2, 3)) == 1 << cpu.RANK[code, L])


def test_syndrome_groups_with_a_ragged_last_group(q, T):
    """N = 1 029 at chunk_bits = 8: a group of 1 024 syndromes and one of 5 (enumr::launch_shape, pinned in tests/test_enumerate_cpu.py)"""
    chains = chains_of(XZZX, 3, 1029)
    want, cls = cpu.twin(T, XZZX, 3, chains, 8)
    same(q.coset_enumerator("xzzx", chains, chunk_bits=8), want, cls, 8)
    assert len({h.tobytes() for h in want}) > 100                               # (many different syndromes: a row in the wrong place would show)


def test_rotated_L5_default_chunk_is_the_twin_and_the_plaquette_enumerator(q, T):
    init = _rand_surf(50 + ORC_CODE[ROTATED], 5, 0.2)                           # (the syndrome tests/test_exact_cpu.py enumerates)
    want, cls = cpu.twin(T, ROTATED, 5, init[None])
    got = q.coset_enumerator("rotated", init)
    same(got, want, cls, 24)
    assert np.array_equal(got["hist"][0].astype(np.int64), _enum(ORC_CODE[ROTATED], init).H)


@pytest.mark.parametrize("code,chunk_bits,ranges", [(XZZX, 10, [(0, 2), ((1 << 14) - 1, 1)]), (ROTATED, 20, [(3, 2), (15, 1)])])
def test_partial_ranges_at_L5(q, T, code, chunk_bits, ranges):
    """two low chunks and the last chunk -- every high basis bit set: the chunk's own product reaches the kernel as an argument"""
    chains = chains_of(code, 5, 2)
    for first, count in ranges:
        want, cls = cpu.twin(T, code, 5, chains, chunk_bits, first, count)
        got = q.coset_enumerator(NAME[code], chains, chunk_bits=chunk_bits, chunks=(first, count))
        same(got, want, cls, 24)
        assert np.all(got["hist"].sum(axis=(2, 3)) == count << chunk_bits)


def test_a_dirty_recycled_block_does_not_leak_into_the_next_call(q, T):
    """the device histogram of a small call is a pooled block that comes back as the last call left it: a full call, then another syndrome, then a
    partial call on the first"""
    a, b = chains_of(XZZX, 3, 1, seed=1), chains_of(XZZX, 3, 1, seed=2)
    wa, ca = cpu.twin(T, XZZX, 3, a)
    wb, cb = cpu.twin(T, XZZX, 3, b)
    assert not np.array_equal(wa, wb)
    same(q.coset_enumerator("xzzx", a), wa, ca, 8)
    same(q.coset_enumerator("xzzx", b), wb, cb, 8)
    c = chains_of(PLANAR, 3, 1, seed=3)
    wc, cc = cpu.twin(T, PLANAR, 3, c)
    same(q.coset_enumerator("planar", c), wc, cc, 12)
    wp, _ = cpu.twin(T, PLANAR, 3, c, 8, 3, 2)
    same(q.coset_enumerator("planar", c, chunk_bits=8, chunks=(3, 2)), wp, cc, 12)


# ------------------------------------------------------------------------------------------------------ method "exact"
def test_generate_exact_from_syndromes_with_corrections(q):
    from qecmc import harness
    params = dict(code="xzzx", size=3, p_error=0.15, noise="depolarizing", method="exact")
    out = harness.generate(params, 300, seed=5, start="syndrome", corrections=True)
    assert "counts" not in out and out["distr"].dtype == np.float64 and out["distr"].shape == (300, 4)
    assert np.allclose(out["distr"].sum(axis=1), 1.0, atol=1e-12)
    assert np.array_equal(out["success_correction"], out["success"])
    assert 0.6 < out["success"].mean() < 1.0 and not out["success"].all()
    # the law does not depend on the start chain: start="error" hides the class behind a logical operator and gets the same distr
    again = harness.generate(params, 300, seed=5)
    assert np.array_equal(again["qubit_matrix"], out["qubit_matrix"]) and np.array_equal(again["distr"], out["distr"])


@pytest.mark.parametrize("noise,extra", [("depolarizing", {}), ("biased", dict(eta=3.0)), ("alpha", dict(alpha=2.0))])
def test_decode_syndromes_exact_is_the_twin_law(q, T, noise, extra):
    from qecmc import exact as ex
    from qecmc import harness
    errors = chains_of(ROTATED, 3, 40)
    defects = harness.syndrome_of("rotated", errors)
    params = dict(code="rotated", size=3, p_error=0.12, noise=noise, method="exact", **extra)
    out = harness.decode_syndromes(params, defects, corrections=True, biased_decoder="alpha")
    hist, _ = cpu.twin(T, ROTATED, 3, out["chains"])
    want = ex.exact_class_probabilities("rotated", None, 0.12, hist=hist, **extra)   # the same NumPy code on equal integers: equal floats
    assert np.array_equal(out["distr"], want) and "counts" not in out
    assert np.array_equal(out["target"], np.argmax(want, axis=1))
    assert np.array_equal(harness.syndrome_of("rotated", out["correction"]), defects)


def test_pteq_does_not_beat_the_exact_decoder(q):
    """paired on one batch (McNemar): a = exact right and PTEQ wrong, b = the reverse.  The exact decoder maximises the success probability, so
    E[a - b] >= 0; b - a <= 5 sqrt(a + b) is 5 sigma of the paired difference."""
    from qecmc import harness
    params = dict(code="xzzx", size=3, p_error=0.15, noise="depolarizing")
    n = 2048
    pteq = harness.generate(params, n, seed=11, steps=2000, conv_criteria=None, device_generation=True)
    exact = harness.generate(dict(params, method="exact"), n, seed=11, device_generation=True)
    assert np.array_equal(pteq["qubit_matrix"], exact["qubit_matrix"]) and np.array_equal(pteq["eq_true"], exact["eq_true"])
    a = int((exact["success"] & ~pteq["success"]).sum())
    b = int((~exact["success"] & pteq["success"]).sum())
    print("exact right / PTEQ wrong: %d, the reverse: %d, success exact %.4f PTEQ %.4f" % (a, b, exact["success"].mean(), pteq["success"].mean()))
    assert b - a <= 5 * np.sqrt(a + b)


def test_planar_sampler_on_the_exact_law(q):
    """4 096 replicas of one planar L = 3 syndrome on exact_class_probabilities: replicas, steps, tops_burn and the acceptance rule of
    tests/test_gpu_stats.py::test_plaquette_exact_L5 (5 sigma + 2e-4 on every class).  The syndrome's two largest class probabilities differ by more
    than 0.01 (tests/test_enumerate_cpu.py checks that on the twin), so the argmax is pinned too."""
    init = random_errors(PLANAR, 3, 8, np.random.default_rng(cpu.PLANAR_PIN_SEED))[cpu.PLANAR_PIN_ROW]
    p = cpu.PLANAR_PIN_P
    P = q.exact_class_probabilities("planar", init, p)[0]
    assert np.sort(P)[-1] - np.sort(P)[-2] > 0.01
    R, steps = 4096, 8000
    res = q.pteq_batch(np.broadcast_to(init, (R,) + init.shape).copy(), p, Nc=3, steps=steps, iters=10, tops_burn=5, seed=6000, code=q.PLANAR)
    ok = res["samples"] > steps // 2
    assert ok.mean() > 0.97
    frac = (res["counts"] / np.maximum(res["samples"], 1)[:, None].astype(np.float64))[ok]
    mean, sem = frac.mean(axis=0), frac.std(axis=0, ddof=1) / np.sqrt(ok.sum())
    print("planar pin: mean", mean, "exact", P, "sem", sem)
    assert np.all(np.abs(mean - P) <= 5 * sem + 2e-4), (mean, P, sem)
    assert mean.argmax() == P.argmax()
