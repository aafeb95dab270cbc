"""Corrections from decoded syndromes on the GPU (qecmc_corrections): the kernel equals the host twin -- the same survey-pick-move-descend body
compiled by g++ (tests/test_corrections_cpu.py pins that one against the oracle) -- bit for bit in all five outputs; it composes on one stream with
the generator and the lift; and through the harness the decoder's answer, applied to the error, leaves a stabilizer exactly where the class labels
agree (success_correction == success on every row)."""
import ctypes as C

import numpy as np
import pytest

import test_corrections_cpu as cpu
import test_syndrome_lift_cpu as lift_cpu
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX

pytestmark = pytest.mark.gpu

SHAPES = [(c, L) for c in (TORIC, XZZX, ROTATED, PLANAR) for L in (3, 5)] + [(TORIC, 9), (ROTATED, 7)]
N = 70                                                                # two wavefronts, the second ragged
BAD = {10: -1, 33: 1000, 66: None}                                    # out-of-range targets (None: ncls), one at least in each wavefront


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return cpu.load_twin()


_batches = {}


def batch(T, code, L, K):
    """70 syndromes of a shape with K candidates each -- the twin lift and copies of it with a logical operator somewhere and a few generators on
    top -- and a target per row, three of them outside [0, ncls); computed once"""
    if (code, L, K) not in _batches:
        rng = np.random.default_rng([3, code, L, K])
        _, defects = lift_cpu.batch(code, L, n=N, seed=4)
        lifted = lift_cpu.twin(T, code, L, defects, 1)[0]
        gens = cpu.generators(code, L)
        cand = np.stack([lifted] * K, axis=1)
        for s in range(N):
            for k in range(1, K):
                m = cpu.apply_kind(code, cand[s, k], int(rng.integers(4 if code == TORIC else 2)), int(rng.integers(L)))
                for g in rng.integers(len(gens), size=3):
                    m = m ^ gens[g].reshape(m.shape)
                cand[s, k] = m
        if K > 1:
            cand[1::5, K - 1] = cand[1::5, K - 2]                      # ties in class and weight
        target = rng.integers(0, cpu.ncls_of(code), size=N).astype(np.int32)
        for s, t in BAD.items():
            target[s] = cpu.ncls_of(code) if t is None else t
        cand.setflags(write=False)
        target.setflags(write=False)
        _batches[code, L, K] = (cand, target)
    return _batches[code, L, K]


def same(got, want):
    for key in ("corrections", "weight", "source", "moved", "status"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("place,descend", cpu.SETTINGS)
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("code,L", SHAPES)
def test_gpu_equals_host_twin(q, T, code, L, K, place, descend):
    cand, target = batch(T, code, L, K)
    want = cpu.twin(T, code, L, cand, target, place, descend)
    got = q.corrections(code, cand if K > 1 else cand[:, 0], target, place=bool(place), descend=bool(descend))
    same(got, want)
    assert want["status"].sum() == len(BAD) and want["moved"].any() and not want["moved"].all()


def test_batch_independence(q, T):
    for code, L in ((TORIC, 5), (ROTATED, 5)):
        cand, target = batch(T, code, L, 3)
        whole = q.corrections(code, cand, target)
        for s in (9, 10, 64, 69):
            alone = q.corrections(code, cand[s:s + 1], target[s:s + 1])
            for key in whole:
                assert np.array_equal(alone[key][0], whole[key][s]), (key, s)


def test_device_pointer_path(q):
    """generate -> syndrome (torch, on the stream) -> lift -> corrections, all enqueued on one non-default stream with torch buffers and ONE
    synchronise at the end: equal to the host-pointer calls, and with the true class as the target every residual is a stabilizer"""
    import torch
    from qecmc import _lib as L_, harness
    code, L, n, p = TORIC, 5, N, 0.12
    nq = 2 * L * L
    lib = L_.lib()
    dev = torch.device("cuda", 0)
    lift, cr = C.c_void_p(), C.c_void_p()
    L_.check(lib.qecmc_lift_create(code, L, C.byref(lift)))
    L_.check(lib.qecmc_corrector_create(code, L, C.byref(cr)))
    try:
        stream = torch.cuda.Stream(device=dev)
        init = torch.empty((n, 2, L, L), dtype=torch.uint8, device=dev)
        raw = torch.empty((n, 2, L, L), dtype=torch.uint8, device=dev)
        eq = torch.empty(n, dtype=torch.int32, device=dev)
        chains = torch.full((n, nq), 9, dtype=torch.uint8, device=dev)
        out = torch.full((n, nq), 9, dtype=torch.uint8, device=dev)
        weight, source = (torch.full((n,), 9, dtype=torch.int32, device=dev) for _ in range(2))
        moved, status = (torch.full((n,), 9, dtype=torch.uint8, device=dev) for _ in range(2))
        bare = torch.full((5, nq), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            sp = C.c_void_p(stream.cuda_stream)
            L_.check(lib.qecmc_generate_syndromes_dev(code, L, n, p / 3, p / 3, p / 3, 0, 11, 0, init.data_ptr(), raw.data_ptr(), eq.data_ptr(), sp))
            yz, xy = raw >= 2, (raw == 1) | (raw == 2)                                      # toric_model.py:58-101
            d0 = yz[:, 0] ^ torch.roll(yz[:, 0], 1, 1) ^ yz[:, 1] ^ torch.roll(yz[:, 1], 1, 2)
            d1 = xy[:, 0] ^ torch.roll(xy[:, 0], -1, 2) ^ xy[:, 1] ^ torch.roll(xy[:, 1], -1, 1)
            defects = torch.stack([d0, d1], dim=1).to(torch.uint8).contiguous()
            L_.check(lib.qecmc_chains_from_syndromes_dev(lift, defects.data_ptr(), n, 1, chains.data_ptr(), None, None, sp))
            L_.check(lib.qecmc_corrections_dev(cr, chains.data_ptr(), eq.data_ptr(), n, 1, 1, 1, out.data_ptr(), weight.data_ptr(), source.data_ptr(),
                                               moved.data_ptr(), status.data_ptr(), sp))
            # the last four outputs are optional
            L_.check(lib.qecmc_corrections_dev(cr, chains.data_ptr(), eq.data_ptr(), 5, 1, 1, 1, bare.data_ptr(), None, None, None, None, sp))
        stream.synchronize()
        raw_h, eq_h = raw.cpu().numpy(), eq.cpu().numpy()
        defects_h = harness.syndrome_of(code, raw_h)
        assert np.array_equal(defects.cpu().numpy().reshape(n, -1), defects_h)
        lifted = q.chains_from_syndromes(code, defects_h, size=L)["chains"]
        assert np.array_equal(chains.cpu().numpy().reshape(lifted.shape), lifted)
        want = q.corrections(code, lifted, eq_h)
        got = dict(corrections=out.cpu().numpy().reshape(lifted.shape), weight=weight.cpu().numpy(), source=source.cpu().numpy(), moved=moved.cpu().numpy(),
                   status=status.cpu().numpy())
        same(got, want)
        assert np.array_equal(bare.cpu().numpy().reshape((5,) + lifted.shape[1:]), want["corrections"][:5])
        residual = raw_h ^ got["corrections"]
        assert not harness.syndrome_of(code, residual).any() and not np.asarray(harness._class_of(code, residual)).any()
    finally:
        lib.qecmc_corrector_destroy(cr)
        lib.qecmc_lift_destroy(lift)


@pytest.mark.parametrize("params,kw", [
    ({"code": "toric", "size": 5, "p_error": 0.08, "noise": "depolarizing"}, dict(steps=200000)),
    ({"code": "rotated", "size": 5, "p_error": 0.05, "noise": "depolarizing"}, dict(steps=3000, conv_criteria=None, tops_burn=0)),
    ({"code": "xzzx", "size": 5, "p_error": 0.05, "noise": "depolarizing"}, dict(steps=3000, conv_criteria=None, tops_burn=0)),
    ({"code": "planar", "size": 5, "p_error": 0.03, "noise": "depolarizing"}, dict(steps=3000, conv_criteria=None, tops_burn=0))])
def test_the_correction_succeeds_exactly_where_the_label_does(q, params, kw):
    """test_decoding_from_the_syndrome_alone's recipe with corrections=True: raw ^ correction is a stabilizer on exactly the rows where
    argmax(distr) == eq_true (that test's own success bars are not repeated here)"""
    from qecmc import harness
    out = harness.generate(params, 256, seed=3, device_generation=True, start="syndrome", corrections=True, **kw)
    print(params["code"], "success", float(np.mean(out["success"])), "mean correction weight", float(np.mean(out["correction_weight"])),
          "mean error weight", float(np.mean((out["qubit_matrix"] != 0).reshape(256, -1).sum(axis=1))))
    assert np.array_equal(out["success_correction"], out["success"])
    defects = harness.syndrome_of(params["code"], out["qubit_matrix"])
    assert np.array_equal(harness.syndrome_of(params["code"], out["correction"]), defects)
    assert np.array_equal(out["correction_weight"], (out["correction"] != 0).reshape(256, -1).sum(axis=1))
    again = harness.decode_syndromes(params, defects, seed=3, corrections=True, **kw)
    assert np.array_equal(again["distr"], out["distr"])
    assert np.array_equal(again["correction"], out["correction"]) and np.array_equal(again["correction_weight"], out["correction_weight"])
    assert np.array_equal(again["target"], np.argmax(out["distr"], axis=1))
    assert np.array_equal(again["correction_source"], np.zeros(256, np.int32))
    assert np.array_equal(again["correction_moved"], np.asarray(harness._class_of(harness._CODES[params["code"]], again["chains"])) != again["target"])
    # the defaults add nothing
    plain = harness.decode_syndromes(params, defects[:64], seed=3, **kw)
    assert not {"target", "correction", "correction_weight", "correction_source", "correction_moved"} & set(plain)


def test_start_error_and_final_states_as_candidates(q):
    from qecmc import harness
    params = {"code": "rotated", "size": 5, "p_error": 0.05, "noise": "depolarizing"}
    kw = dict(steps=1000, conv_criteria=None, tops_burn=0)
    # start="error": the candidate is the seed configuration (the error with a random logical operator on top)
    out = harness.generate(params, 128, seed=5, corrections=True, **kw)
    assert np.array_equal(out["success_correction"], out["success"])
    assert "correction" not in harness.generate(params, 8, seed=5, **kw)
    with pytest.raises(ValueError):
        harness.generate(dict(params, method="PTDC"), 4, seed=5, corrections=True, steps=100)
    # the Nc final rung states as further candidates, where the route returns them
    defects = harness.syndrome_of("rotated", out["qubit_matrix"])
    lone = harness.decode_syndromes(params, defects, seed=5, corrections=True, **kw)
    more = harness.decode_syndromes(params, defects, seed=5, corrections=True, correction_candidates="states", **kw)
    assert np.array_equal(more["distr"], lone["distr"]) and np.array_equal(more["target"], lone["target"])
    assert np.array_equal(harness.syndrome_of("rotated", more["correction"]), defects)
    assert np.array_equal(np.asarray(harness._class_of(harness._CODES["rotated"], more["correction"])), more["target"])
    assert more["correction_source"].max() <= 5 and (more["correction_source"] > 0).any()
    assert more["correction_moved"].sum() <= lone["correction_moved"].sum()                 # more candidates: a target class is found at least as often
    with pytest.raises(ValueError, match="conv_criteria='error_based'"):
        harness.decode_syndromes(params, defects[:8], seed=5, corrections=True, correction_candidates="states", steps=1000)
