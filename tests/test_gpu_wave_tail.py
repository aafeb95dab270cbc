"""The step tail of the fixed-length scan = "wave" kernels (csrc/ladder_wu.hpp: the exchange of the states, the swap cascade, the bookkeeping), bit for
bit against the oracle's scan = 3 in both of its forms: the cascade walked once per workgroup by the top rung's wave (what wave_cascade_once() chooses at 5, 6 and 7 rungs where four workgroups fit a CU), and replayed by every wave (the other shapes, and every
shape under QECMC_FLAG_NO_SSW, flags bit 8).  The shapes are picked for the tail: 2, 3 and 8 rungs (512-thread workgroups, replay either way), 5, 6
and 7 (once / replay), 9 and 16 (1 024); every state width 4 / 8 / 12 / 16 words in both forms and a 32-word one (which keeps its two-halves tail);
iters 1, 7, 10; ragged batches; a run resumed at step0 != 0; and ladders whose top pair is kSwapFast = 64 or more errors apart, which look their swap
threshold up in the plan's table in global memory instead of the LDS rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SSW = 8
FORMS = [pytest.param(0, id="chosen"), pytest.param(NO_SSW, id="replay")]


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _codes(q, orc, name):
    return {"toric": (q.TORIC, orc.TORIC), "xzzx": (q.XZZX, orc.XZZX), "rotated": (q.ROTATED, orc.ROTATED), "planar": (q.PLANAR, orc.PLANAR)}[name]


def _init(rng, name, N, L, p):
    shape = (N, 2, L, L) if name in ("toric", "planar") else (N, L, L)
    init = (rng.integers(1, 4, size=shape) * (rng.random(shape) < p)).astype(np.uint8)
    if name == "planar":
        init[:, 1, -1, :] = 0; init[:, 1, :, -1] = 0
    return init


def _same(got, ref, ncls):
    assert np.array_equal(got["states"], ref["states"])
    assert np.array_equal(got["counts"], ref["counts"][:, :ncls])
    assert np.array_equal(got["samples"], ref["samples"].astype(np.uint32))
    assert np.array_equal(got["tops0"], ref["tops0"].astype(np.uint32))


CASES = [  # name, L, Nc, N, steps, iters, p, first_syndrome                         words of a rung, threads
    ("toric", 3, 2, 70, 3000, 10, 0.10, 0),          # 2 -> 4,  512: one pair; two workgroups, the second ragged
    ("toric", 5, 3, 5, 3000, 7, 0.10, 64),           # 4,       512; iters 7
    ("toric", 7, 8, 6, 2000, 10, 0.12, 0),           # 7 -> 8,  512
    ("toric", 9, 8, 130, 4000, 10, 0.15, 128),       # 11 -> 12, 512: config 2's kernel; three workgroups, the last ragged
    ("toric", 9, 8, 3, 1500, 1, 0.15, 0),            # ... iters 1
    ("toric", 11, 4, 4, 1000, 7, 0.15, 0),           # 16,      512: four workgroups of 16 words fit a CU
    ("toric", 11, 8, 3, 600, 10, 0.18, 0),           # 16,      512: fewer than four fit -- the replay either way
    ("toric", 9, 9, 3, 800, 10, 0.15, 0),            # 12,      1 024
    ("toric", 9, 16, 2, 500, 7, 0.15, 64),           # 12,      1 024: sixteen rungs, four blocks of swap uniforms
    ("toric", 5, 16, 66, 600, 10, 0.10, 0),          # 4,       1 024; ragged
    ("xzzx", 9, 8, 5, 1500, 10, 0.15, 0),            # 6 -> 8,  512
    ("rotated", 13, 8, 3, 800, 7, 0.17, 0),          # 11 -> 12, 512
    ("planar", 5, 5, 4, 1500, 10, 0.12, 0),          # 4,       512
    ("toric", 15, 8, 3, 400, 10, 0.18, 0),           # 29 -> 32: the 32-word kernel (the state through the buffer in two halves)
    # 5, 6, 7 rungs: the cascade once per workgroup unless flag 8 asks for the replay
    ("toric", 5, 5, 70, 2000, 10, 0.10, 64),         # 4 words; ragged
    ("toric", 7, 6, 5, 2000, 7, 0.12, 0),            # 8 words; two blocks of swap uniforms (five pairs)
    ("toric", 9, 7, 130, 2000, 10, 0.15, 0),         # 12 words; ragged
    ("toric", 9, 5, 3, 1500, 1, 0.15, 0),            # 12 words; iters 1: one block of swap uniforms (four pairs)
    ("toric", 11, 5, 4, 1000, 10, 0.15, 0),          # 16 words
    ("xzzx", 9, 6, 5, 1500, 10, 0.15, 0), ("rotated", 13, 7, 3, 800, 10, 0.17, 0),
]


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("name,L,Nc,N,steps,iters,p,first", CASES)
def test_wave_tail_bit_exact(q, orc, name, L, Nc, N, steps, iters, p, first, flags):
    rng = np.random.default_rng(1000 * L + 16 * Nc + iters)
    code, ocode = _codes(q, orc, name)
    init = _init(rng, name, N, L, p)
    # (tops_burn = 0: the class histogram is booked from the first step on, whether or not a run this short brings a state down from the top rung)
    kw = dict(steps=steps, iters=iters, tops_burn=0, seed=91, first_syndrome=first)
    got = q.pteq_batch(init, p, Nc=Nc, code=code, scan="wave", return_states=True, flags=flags, **kw)
    ref = orc.pteq_batch(ocode, init, p, Nc, return_states=True, scan=3, **kw)
    _same(got, ref, 16 if name == "toric" else 4)


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("L,Nc,steps", [(9, 2, 40), (11, 2, 30), (9, 8, 25), (9, 6, 25)])
def test_wave_tail_far_pairs_take_the_plans_table(q, orc, L, Nc, steps, flags):
    """Two rungs at p = 0.05: the top rung (p = 0.75) drifts to about three quarters of the qubits in error while the bottom one stays near its
    syndrome's weight, so the pair is 64 or more errors apart from the first few steps on and every swap test takes the plan's table.  Eight (replay)
    and six (once per workgroup) rungs at config 2's own p take it in their first steps only.  (The premise is checked on the oracle's states, not assumed.)"""
    sys.path.insert(0, ROOT)
    import bench
    p = 0.05 if Nc == 2 else 0.15
    init = bench.synth_batch(64, L, p, 7)
    kw = dict(iters=10, tops_burn=1, seed=7)
    if Nc == 2:
        mid = orc.pteq_batch(orc.TORIC, init, p, Nc, 8, return_states=True, scan=3, **kw)["states"]
        n = (mid.reshape(64, Nc, -1) != 0).sum(axis=2)
        assert (n[:, 1] - n[:, 0] >= 64).all(), "the shape no longer drives the top pair kSwapFast apart"
    got = q.pteq_batch(init, p, Nc=Nc, scan="wave", return_states=True, steps=steps, flags=flags, **kw)
    ref = orc.pteq_batch(orc.TORIC, init, p, Nc, steps, return_states=True, scan=3, **kw)
    _same(got, ref, 16)


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("L,Nc,N,chunks,iters", [(9, 8, 70, (37, 1, 62), 10), (9, 7, 70, (37, 1, 62), 10), (5, 3, 5, (50, 50), 7), (9, 9, 3, (20, 30), 10)])
def test_wave_tail_resumed_run_equals_one_long_run(q, orc, L, Nc, N, chunks, iters, flags):
    """qecmc_pteq_resume_dev with scan = wave: chunks continued from device-resident states at step0 != 0 (also inside a pick window: 37 is no multiple
    of the 12 steps a window of iters = 10 serves) reproduce the oracle's single run"""
    import torch
    from qecmc import _lib as L_
    rng = np.random.default_rng(L + Nc)
    p, first = 0.15, 64
    init = _init(rng, "toric", N, L, p)
    nq = 2 * L * L
    dev = torch.device("cuda", 0)
    states = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(init.reshape(N, 1, nq), (N, Nc, nq)))).to(dev)
    fl = np.zeros((N, Nc), dtype=np.uint8); fl[:, -1] = 1
    flg = torch.from_numpy(fl).to(dev)
    tops0 = torch.zeros(N, dtype=torch.int32, device=dev)
    counts = torch.zeros((N, 16), dtype=torch.int32, device=dev)
    samples = torch.zeros(N, dtype=torch.int32, device=dev)
    done = 0
    for steps in chunks:
        pl = C.c_void_p()
        pr = L_.make_params(code=L_.TORIC, L=L, Nc=Nc, p=p, p_logical=0.5, iters=iters, steps=steps, tops_burn=1, seed=33, scan=L_.SCAN_WAVE, flags=flags)
        L_.check(L_.lib().qecmc_plan_create(pr, C.byref(pl)))
        try:
            L_.check(L_.lib().qecmc_pteq_resume_dev(pl, states.data_ptr(), flg.data_ptr(), tops0.data_ptr(), N, first, done, counts.data_ptr(),
                                                    samples.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            torch.cuda.synchronize()
        finally:
            L_.lib().qecmc_plan_destroy(pl)
        done += steps
    ref = orc.pteq_batch(orc.TORIC, init, p, Nc, done, iters=iters, tops_burn=1, seed=33, first_syndrome=first, return_states=True, scan=3)
    got = dict(states=states.cpu().numpy().reshape((N, Nc) + init.shape[1:]), counts=counts.cpu().numpy().view(np.uint32),
               samples=samples.cpu().numpy().view(np.uint32), tops0=tops0.cpu().numpy().view(np.uint32))
    _same(got, ref, 16)
