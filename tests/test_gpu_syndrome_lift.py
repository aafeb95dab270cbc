"""Start chains from bare syndromes on the GPU (qecmc_chains_from_syndromes): the kernel equals the host twin -- the same lift-and-descend body
compiled by g++ (tests/test_syndrome_lift_cpu.py pins that one against the oracle) -- bit for bit; the chains go straight into the sampler; and
decoding from nothing but the syndrome clears the success bars of test_gpu_stats.py::test_harness_generate_decodes_low_noise."""
import ctypes as C

import numpy as np
import pytest

import test_syndrome_lift_cpu as cpu
from oracle import oracle as orc
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX

pytestmark = pytest.mark.gpu

SHAPES = [(c, L) for c in (TORIC, XZZX, ROTATED, PLANAR) for L in (3, 5)] + [(TORIC, 4), (TORIC, 15), (ROTATED, 21)]   # toric 15: 29 state words, rotated 21: 28
N = 70                                                                # two wavefronts, the second ragged


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return cpu.load_twin()


_batches = {}


def defects_of(code, L):
    """70 syndromes of a shape, two of them none of the code where the code has such (rows 10 and 66: one in each wavefront; every defect
    pattern of the planar code is a syndrome); computed once"""
    if (code, L) not in _batches:
        _, d = cpu.batch(code, L, n=N, seed=2)
        if code == TORIC:
            d[10, 3] ^= 1                                             # an odd number of defects in a component of the torus
            d[66, L * L + 1] ^= 1
        elif code != PLANAR:
            d[10, 0] = 1                                              # corners of the (L+1)^2 grid are no checks
            d[66, (L + 1) * (L + 1) - 1] = 1
        d.setflags(write=False)
        _batches[code, L] = d
    return _batches[code, L]


def gpu_lift(q, code, L, defects, descend):
    res = q.chains_from_syndromes(code, defects, descend=bool(descend), size=L)
    return res["chains"], res["status"], res["weight"]


@pytest.mark.parametrize("descend", [0, 1])
@pytest.mark.parametrize("code,L", SHAPES)
def test_gpu_equals_host_twin(q, T, code, L, descend):
    d = defects_of(code, L)
    want = cpu.twin(T, code, L, d, descend)
    got = gpu_lift(q, code, L, d, descend)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert want[1].sum() == (0 if code == PLANAR else 2)


def test_batch_independence(q):
    for code, L in ((TORIC, 5), (ROTATED, 5)):
        d = defects_of(code, L)
        whole = gpu_lift(q, code, L, d, 1)
        alone = gpu_lift(q, code, L, d[13:21], 1)
        for a, w in zip(alone, whole):
            assert np.array_equal(a, w[13:21])


def test_device_pointer_path(q):
    """qecmc_lift_create once, two launches of different N on a non-default stream: equal to the host-pointer call"""
    import torch
    from qecmc import _lib as L_
    code, L = TORIC, 5
    d = defects_of(code, L)
    want = gpu_lift(q, code, L, d, 1)
    dev = torch.device("cuda", 0)
    lift = C.c_void_p()
    L_.check(L_.lib().qecmc_lift_create(code, L, C.byref(lift)))
    try:
        stream = torch.cuda.Stream(device=dev)
        d_dev = torch.from_numpy(np.array(d)).to(dev)
        outs = []
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            for n in (N, 5):
                chains = torch.full((n, 2 * L * L), 9, dtype=torch.uint8, device=dev)
                status = torch.full((n,), 9, dtype=torch.uint8, device=dev)
                weight = torch.full((n,), 9, dtype=torch.int32, device=dev)
                L_.check(L_.lib().qecmc_chains_from_syndromes_dev(lift, d_dev.data_ptr(), n, 1, chains.data_ptr(), status.data_ptr(), weight.data_ptr(),
                                                                  C.c_void_p(stream.cuda_stream)))
                outs.append((n, chains, status, weight))
            # status and weight are optional
            bare = torch.full((5, 2 * L * L), 9, dtype=torch.uint8, device=dev)
            L_.check(L_.lib().qecmc_chains_from_syndromes_dev(lift, d_dev.data_ptr(), 5, 1, bare.data_ptr(), None, None, C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        for n, chains, status, weight in outs:
            assert np.array_equal(chains.cpu().numpy().reshape(n, 2, L, L), want[0][:n])
            assert np.array_equal(status.cpu().numpy(), want[1][:n]) and np.array_equal(weight.cpu().numpy(), want[2][:n])
        assert np.array_equal(bare.cpu().numpy().reshape(5, 2, L, L), want[0][:5])
    finally:
        L_.lib().qecmc_lift_destroy(lift)


def test_chains_feed_the_sampler(q, T):
    from qecmc import harness
    for code, L in ((TORIC, 5), (XZZX, 5), (ROTATED, 5), (PLANAR, 5)):
        d = defects_of(code, L)
        chains, status, _ = gpu_lift(q, code, L, d, 1)
        ok = status == 0
        assert np.array_equal(harness.syndrome_of(code, chains)[ok], d[ok])       # the device's own syndrome kernel
    # ... and as `init` of the sampler: the same ladders as the oracle runs from the twin's chains
    d = defects_of(TORIC, 5)
    chains = gpu_lift(q, TORIC, 5, d, 1)[0]
    got = q.pteq_batch(chains, p=0.15, Nc=4, steps=200, tops_burn=0, return_states=True)
    ref = orc.pteq_batch(orc.TORIC, cpu.twin(T, TORIC, 5, d, 1)[0], 0.15, 4, 200, tops_burn=0, return_states=True)
    assert np.array_equal(got["counts"], ref["counts"])
    assert np.array_equal(got["samples"], ref["samples"].astype(np.uint32))
    assert np.array_equal(got["tops0"], ref["tops0"].astype(np.uint32))
    assert np.array_equal(got["states"], ref["states"])


@pytest.mark.parametrize("params,kw,bar", [
    ({"code": "toric", "size": 5, "p_error": 0.08, "noise": "depolarizing"}, dict(steps=200000), 0.75),
    ({"code": "rotated", "size": 5, "p_error": 0.05, "noise": "depolarizing"}, dict(steps=3000, conv_criteria=None, tops_burn=0), 0.9),
    ({"code": "xzzx", "size": 5, "p_error": 0.05, "noise": "depolarizing"}, dict(steps=3000, conv_criteria=None, tops_burn=0), 0.9),
    ({"code": "planar", "size": 5, "p_error": 0.03, "noise": "depolarizing"}, dict(steps=3000, conv_criteria=None, tops_burn=0), 0.9)])
def test_decoding_from_the_syndrome_alone(q, params, kw, bar):
    """test_harness_generate_decodes_low_noise's recipe and bars with start="syndrome": only syndrome(raw) reaches the decoder"""
    from qecmc import harness
    out = harness.generate(params, 256, seed=3, device_generation=True, start="syndrome", **kw)
    rate = float(np.mean(out["success"]))
    print(params["code"], "success from lifted starts", rate, "mean steps", float(np.mean(out["steps_done"])))
    assert rate > bar
    defects = harness.syndrome_of(params["code"], out["qubit_matrix"])
    again = harness.decode_syndromes(params, defects, seed=3, **kw)
    assert not again["status"].any()
    assert np.array_equal(again["distr"], out["distr"])
    assert np.array_equal(again["steps_done"], out["steps_done"])
    with pytest.raises(ValueError):
        harness.generate(dict(params, method="PTDC"), 4, seed=3, start="syndrome", steps=100)
