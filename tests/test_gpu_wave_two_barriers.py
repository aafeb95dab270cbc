"""The walked swap cascade of the scan = "wave" kernels as a step of TWO barriers (csrc/ladder_wu.hpp, the lean tail: every wave publishes its record in
front of the step's first barrier, the top rung's wave walks right behind it and every wave's state stores go out in the walk's shadow), and rung 0's
booking -- tops0, the class histogram, samples -- by whichever wave the build lets book (kWuTopBooks: wave 0, or the walker from the record its chain
ends with), bit for bit against the oracle's scan = 3: states, counts, samples and tops0.  Every case runs in three forms: the one the launch chooses (wave_cascade_mode(), csrc/kernel_choice.hpp),
QECMC_FLAG_NO_SPREAD (flags bit 16: LadderArgs::wu_once 1 at eight rungs) and QECMC_FLAG_NO_SSW (bit 8: the replay, which keeps its step and wave 0's
booking).  A race between a record, a bound or a state store and its reader shows as a mismatch, so the shapes are several co-resident workgroups and many
steps, not large lattices: config 2's kernel over four workgroups, the last one ragged; runs of one, two and three steps; 5, 6 and 7 rungs at 4 and 8 state
words (the walker's dropped loads then fall into rows that are being stored into); eight rungs at 4 and 8 words; the three other codes; the general loop
(walked with no draw in the walk's shadow); a run resumed in chunks that end inside a pick window and inside a priority period, across which tops0 and the
flags travel; the booking under tops_burn 0 and 2, with the flag never and always set by the top rung's moves, and with xzzx's class fold; and shapes
whose step must not have changed.  The oracle's result of a case is computed once and shared by the forms."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

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
    kw = dict(steps=steps, iters=iters, tops_burn=0, seed=163, first_syndrome=first)
    got = q.pteq_batch(init, p, Nc=Nc, code=code, scan="wave", return_states=True, flags=flags, **kw)
    ref = _ref(("case", name, L, Nc, N, steps, iters), lambda: orc.pteq_batch(ocode, init, p, Nc, return_states=True, scan=3, **kw))
    _same(got, ref, 16 if name == "toric" else 4)
    assert int(got["counts"].sum()) == N * steps        # every step of every ladder is booked exactly once, by whichever wave books


CASES = [  # name, L, Nc, N, steps, iters, p, first_syndrome                        words of a rung
    ("toric", 9, 8, 194, 600, 10, 0.15, 128),        # 12: config 2's kernel; four workgroups, the last ragged
    ("toric", 9, 8, 5, 1, 10, 0.15, 0),              # ... one step: the first-step path, and the last step at once
    ("toric", 9, 8, 5, 2, 10, 0.15, 0),              # ... two: the first hand-over
    ("toric", 9, 8, 5, 3, 10, 0.15, 0),              # ... three: a step between two steps of the loop, then the last
    ("toric", 5, 5, 70, 400, 10, 0.10, 64),          # 4 words, five rungs: three dropped record loads fall into the top rung's region
    ("toric", 5, 6, 70, 400, 10, 0.10, 64),          # ... six: two
    ("toric", 5, 7, 70, 400, 10, 0.10, 64),          # ... seven: one
    ("toric", 7, 5, 70, 400, 10, 0.12, 0),           # 8 words, five rungs
    ("toric", 7, 6, 70, 400, 10, 0.12, 0),           # ... six
    ("toric", 7, 7, 70, 400, 10, 0.12, 0),           # ... seven
    ("toric", 3, 8, 70, 400, 10, 0.10, 0),           # eight rungs at 2 -> 4 words
    ("toric", 7, 8, 70, 400, 10, 0.12, 64),          # ... at 7 -> 8
    ("xzzx", 9, 8, 70, 400, 10, 0.15, 0),            # 6 -> 8
    ("rotated", 13, 8, 70, 300, 10, 0.17, 0),        # 11 -> 12
    ("planar", 5, 8, 70, 400, 10, 0.12, 0),          # 4
    ("toric", 7, 6, 70, 400, 7, 0.12, 0),            # the general loop (iters 7): walked, the waves below the top draw a block of swap words each and have
                                                     # the state stores alone in the walk's shadow
]


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("name,L,Nc,N,steps,iters,p,first", CASES)
def test_wave_two_barriers_bit_exact(q, orc, name, L, Nc, N, steps, iters, p, first, flags):
    _run_case(q, orc, name, L, Nc, N, steps, iters, p, first, flags)


UNCHANGED = [  # shapes whose step did not change: the form the launch chooses only
    ("toric", 5, 4, 70, 400, 10, 0.10, 64),          # four rungs: the replay
    ("toric", 5, 9, 70, 300, 10, 0.10, 0),           # nine rungs: the 1 024-thread kernel
    ("toric", 11, 8, 5, 300, 10, 0.18, 0),           # 16 words: fewer than four workgroups fit a CU -- the replay
]


@pytest.mark.parametrize("name,L,Nc,N,steps,iters,p,first", UNCHANGED)
def test_wave_two_barriers_leaves_the_other_shapes_alone(q, orc, name, L, Nc, N, steps, iters, p, first):
    _run_case(q, orc, name, L, Nc, N, steps, iters, p, first, 0)


def _ladders(orc, ocode, name, init, p, Nc, steps, p_logical, first, seed, tops_burn):
    """the oracle's ladders one by one (scan = 3) under a p_logical of the caller's: the booking rule of decoders.py:60-67 restated on Ladder.step"""
    N = init.shape[0]
    ncls = 16 if name == "toric" else 4
    counts = np.zeros((N, ncls), np.uint32); samples = np.zeros(N, np.uint64); tops0 = np.zeros(N, np.uint64)
    states = np.zeros((N, Nc) + init.shape[1:], np.uint8)
    for l in range(N):
        ld = orc.Ladder(ocode, init[l], p, Nc, p_logical, scan=3)
        r = orc.Rng.philox(seed, first + l)
        for _ in range(steps):
            ld.step(10, r)
            if ld.tops0 >= tops_burn:
                counts[l, orc.surf_eq_class(ocode, ld.states[0]) if name != "toric" else orc.toric_eq_class(ld.states[0])] += 1
                samples[l] += 1
        tops0[l] = ld.tops0
        states[l] = ld.states
    return dict(states=states, counts=counts, samples=samples, tops0=tops0)


BOOKING = [  # name, L, Nc, p
    ("toric", 5, 8, 0.30),                           # the walk on bounds the lower waves found (a rate at which the flag reaches rung 0 within the run)
    ("toric", 5, 6, 0.30),                           # ... on the top wave's own
    ("xzzx", 5, 8, 0.12),                            # the class fold: the histogram's row is v ^ (v >> 1) of the record's class field
]


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("p_logical", [0.0, 1.0])
@pytest.mark.parametrize("tops_burn", [0, 2])
@pytest.mark.parametrize("name,L,Nc,p", BOOKING)
def test_wave_two_barriers_booking(q, orc, name, L, Nc, p, tops_burn, p_logical, flags):
    """tops0, the burn-in test, the histogram row and samples, whichever wave books them: with the burn-in over at once and over only after two arrivals
    of the flag, under a top rung that never and that always proposes a logical operator"""
    N, steps, first, seed = 70, 400, 64, 167
    rng = np.random.default_rng(100 * L + Nc)
    code, ocode = _codes(q, orc, name)
    init = _init(rng, name, N, L, p)
    got = q.pteq_batch(init, p, Nc=Nc, code=code, scan="wave", p_logical=p_logical, return_states=True, steps=steps, iters=10, tops_burn=tops_burn,
                       seed=seed, first_syndrome=first, flags=flags)
    ref = _ref(("book", name, L, Nc, tops_burn, p_logical), lambda: _ladders(orc, ocode, name, init, p, Nc, steps, p_logical, first, seed, tops_burn))
    _same(got, ref, 16 if name == "toric" else 4)
    assert np.array_equal(got["counts"].sum(axis=1), got["samples"])
    if tops_burn == 0:
        assert int(got["counts"].sum()) == N * steps
    else:
        assert (ref["tops0"] >= tops_burn).any() and (ref["samples"] < steps).any(), "the shape no longer has a burn-in to test"


@pytest.mark.parametrize("flags", FORMS)
def test_wave_two_barriers_resumed_run_equals_one_long_run(q, orc, flags):
    """qecmc_pteq_resume_dev at config 2's kernel in chunks of 37, 1, 29 and 33 steps, equal to the one run of 100: the chunks end at steps 37, 38 and 67,
    multiples neither of a pick window (12 steps) nor of a priority period (16), every chunk takes the first-step path, and tops0 and the flags cross every
    boundary -- tops0 into the wave that books"""
    import torch
    from qecmc import _lib as L_
    L, Nc, N, chunks, iters = 9, 8, 70, (37, 1, 29, 33), 10
    assert all(b % 12 and b % 16 for b in np.cumsum(chunks)[:-1])
    rng = np.random.default_rng(L + Nc + 5)
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
        pr = L_.make_params(code=L_.TORIC, L=L, Nc=Nc, p=p, p_logical=0.5, iters=iters, steps=steps, tops_burn=2, seed=43, scan=L_.SCAN_WAVE, flags=flags)
        L_.check(L_.lib().qecmc_plan_create(pr, C.byref(pl)))
        try:
            L_.check(L_.lib().qecmc_pteq_resume_dev(pl, states.data_ptr(), flg.data_ptr(), tops0.data_ptr(), N, first, done, counts.data_ptr(),
                                                    samples.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            torch.cuda.synchronize()
        finally:
            L_.lib().qecmc_plan_destroy(pl)
        done += steps
    ref = _ref("resumed", lambda: orc.pteq_batch(orc.TORIC, init, p, Nc, done, iters=iters, tops_burn=2, seed=43, first_syndrome=first, return_states=True, scan=3))
    got = dict(states=states.cpu().numpy().reshape((N, Nc) + init.shape[1:]), counts=counts.cpu().numpy().view(np.uint32),
               samples=samples.cpu().numpy().view(np.uint32), tops0=tops0.cpu().numpy().view(np.uint32))
    _same(got, ref, 16)
