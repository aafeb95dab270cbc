"""The walked swap cascade of the scan = "wave" kernels with the bounds spread over the waves below the top (csrc/ladder_wu.hpp, LadderArgs::wu_once == 2:
the top rung's wave draws the NEXT step's swap words and stores them raw behind its walk, the wave of slot s turns the word of pair s into the bound in
place, the first step's words are stored in front of one barrier outside the step loop), bit for bit against the oracle's scan = 3: states, counts,
samples and tops0.  Every case runs in three forms: the one the launch chooses (wave_cascade_mode(), csrc/kernel_choice.hpp), QECMC_FLAG_NO_SPREAD (flags
bit 16: the top wave finds every bound) and QECMC_FLAG_NO_SSW (bit 8: the replay).  The shapes are picked for what the change can break: config 2's
kernel over three workgroups, the last one ragged; runs of one, two and three steps (the first-step path, the first hand-over, the draw nobody reads); one
block of four pairs, a second block of one and of two pairs; 4, 8 and 16 state words at eight rungs (16: the replay either way); the three other codes;
ladders whose top pairs are kSwapFast = 64 or more errors apart (a lower wave's own walk into the plan's table decides); a run resumed in chunks, each of
which takes the first-step path; and shapes that must not have changed (the replay at four rungs, the general loop, more than eight rungs).  The oracle's
result of a case is computed once and shared by the forms."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SSW, NO_SPREAD = 8, 16
FORMS = [pytest.param(0, id="chosen"), pytest.param(NO_SPREAD, id="top-bounds"), pytest.param(NO_SSW, id="replay")]
_REF = {}


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


def _ref(key, make):
    """the oracle's result of a case: computed by the first form that asks, read (never written) by the others"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _same(got, ref, ncls):
    assert np.array_equal(got["states"], ref["states"])
    assert np.array_equal(got["counts"], ref["counts"][:, :ncls])
    assert np.array_equal(got["samples"], ref["samples"].astype(np.uint32))
    assert np.array_equal(got["tops0"], ref["tops0"].astype(np.uint32))


def _run_case(q, orc, name, L, Nc, N, steps, iters, p, first, flags):
    rng = np.random.default_rng(1000 * L + 16 * Nc + iters + steps)
    code, ocode = _codes(q, orc, name)
    init = _init(rng, name, N, L, p)
    # (tops_burn = 0: the class histogram is booked from the first step on)
    kw = dict(steps=steps, iters=iters, tops_burn=0, seed=151, first_syndrome=first)
    got = q.pteq_batch(init, p, Nc=Nc, code=code, scan="wave", return_states=True, flags=flags, **kw)
    ref = _ref(("case", name, L, Nc, N, steps, iters), lambda: orc.pteq_batch(ocode, init, p, Nc, return_states=True, scan=3, **kw))
    _same(got, ref, 16 if name == "toric" else 4)


CASES = [  # name, L, Nc, N, steps, iters, p, first_syndrome                        words of a rung
    ("toric", 9, 8, 130, 600, 10, 0.15, 128),        # 12: config 2's kernel; three workgroups, the last ragged
    ("toric", 9, 8, 5, 1, 10, 0.15, 0),              # ... one step: the first-step path, and the last step at once
    ("toric", 9, 8, 5, 2, 10, 0.15, 0),              # ... two: the first hand-over
    ("toric", 9, 8, 5, 3, 10, 0.15, 0),              # ... three: a hand-over between two steps of the loop; the last draw is read by nobody
    ("toric", 5, 5, 70, 400, 10, 0.10, 64),          # 4; five rungs: one block of four pairs; ragged
    ("toric", 7, 6, 5, 400, 10, 0.12, 0),            # 8; six rungs: a second block of one pair
    ("toric", 7, 7, 70, 400, 10, 0.12, 0),           # 8; seven rungs: ... of two; ragged
    ("toric", 3, 8, 6, 400, 10, 0.10, 0),            # 2 -> 4 words at eight rungs
    ("toric", 7, 8, 6, 400, 10, 0.12, 64),           # 7 -> 8
    ("toric", 11, 8, 3, 300, 10, 0.18, 0),           # 16: fewer than four workgroups fit a CU -- the replay either way
    ("xzzx", 9, 8, 5, 400, 10, 0.15, 0),             # 6 -> 8
    ("rotated", 13, 8, 3, 300, 10, 0.17, 0),         # 11 -> 12
    ("planar", 5, 8, 4, 400, 10, 0.12, 0),           # 4
]


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("name,L,Nc,N,steps,iters,p,first", CASES)
def test_wave_spread_bounds_bit_exact(q, orc, name, L, Nc, N, steps, iters, p, first, flags):
    _run_case(q, orc, name, L, Nc, N, steps, iters, p, first, flags)


UNCHANGED = [  # shapes whose code did not change: the form the launch chooses only
    ("toric", 5, 4, 5, 400, 10, 0.10, 64),           # four rungs: the replay
    ("toric", 7, 6, 5, 400, 7, 0.12, 0),             # six rungs on the general loop (iters 7): walked, the waves below the top draw a block each
    ("toric", 5, 9, 5, 300, 10, 0.10, 0),            # nine rungs: the 1 024-thread kernel
]


@pytest.mark.parametrize("name,L,Nc,N,steps,iters,p,first", UNCHANGED)
def test_wave_spread_bounds_leaves_the_other_kernels_alone(q, orc, name, L, Nc, N, steps, iters, p, first):
    _run_case(q, orc, name, L, Nc, N, steps, iters, p, first, 0)


@pytest.mark.parametrize("flags", FORMS)
def test_wave_spread_bounds_far_pairs_walk_into_the_plans_table(q, orc, flags):
    """config 2's own syndromes: in the first steps of a run the pairs next to the top rung are kSwapFast = 64 or more errors apart, a distance only a
    bound found in the plan's table in global memory lets pass -- here by the walk of the wave below the pair (the premise is checked on the oracle's
    states)"""
    sys.path.insert(0, ROOT)
    import bench
    L, Nc, p = 9, 8, 0.15
    init = bench.synth_batch(64, L, p, 7)
    kw = dict(iters=10, tops_burn=1, seed=7)

    def make():
        mid = orc.pteq_batch(orc.TORIC, init, p, Nc, 2, return_states=True, scan=3, **kw)["states"]
        n = (mid.reshape(64, Nc, -1) != 0).sum(axis=2)
        assert (np.abs(n[:, 1:] - n[:, :-1]) >= 64).any(), "the shape no longer drives a pair of neighbouring rungs kSwapFast apart"
        return orc.pteq_batch(orc.TORIC, init, p, Nc, 25, return_states=True, scan=3, **kw)

    got = q.pteq_batch(init, p, Nc=Nc, scan="wave", return_states=True, steps=25, flags=flags, **kw)
    _same(got, _ref("far", make), 16)


@pytest.mark.parametrize("flags", FORMS)
def test_wave_spread_bounds_resumed_run_equals_one_long_run(q, orc, flags):
    """qecmc_pteq_resume_dev at config 2's kernel in chunks of 37, 1 and 62 steps, equal to the one run of 100: every chunk stores its first step's words in
    front of its loop, and the one-step chunk's first step is its last"""
    import torch
    from qecmc import _lib as L_
    L, Nc, N, chunks, iters = 9, 8, 70, (37, 1, 62), 10
    rng = np.random.default_rng(L + Nc + 3)
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
        pr = L_.make_params(code=L_.TORIC, L=L, Nc=Nc, p=p, p_logical=0.5, iters=iters, steps=steps, tops_burn=1, seed=41, scan=L_.SCAN_WAVE, flags=flags)
        L_.check(L_.lib().qecmc_plan_create(pr, C.byref(pl)))
        try:
            L_.check(L_.lib().qecmc_pteq_resume_dev(pl, states.data_ptr(), flg.data_ptr(), tops0.data_ptr(), N, first, done, counts.data_ptr(),
                                                    samples.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            torch.cuda.synchronize()
        finally:
            L_.lib().qecmc_plan_destroy(pl)
        done += steps
    ref = _ref("resumed", lambda: orc.pteq_batch(orc.TORIC, init, p, Nc, done, iters=iters, tops_burn=1, seed=41, first_syndrome=first, return_states=True, scan=3))
    got = dict(states=states.cpu().numpy().reshape((N, Nc) + init.shape[1:]), counts=counts.cpu().numpy().view(np.uint32),
               samples=samples.cpu().numpy().view(np.uint32), tops0=tops0.cpu().numpy().view(np.uint32))
    _same(got, ref, 16)
