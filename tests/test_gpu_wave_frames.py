"""scan = "wave", the top rung's moves as frames (csrc/wu_frames.hpp, csrc/ladder_wu.hpp): the fixed-length kernels of up to 16 state words with iters = 10
build the top rung's ten moves of every ladder step of a pick window (12 steps) as one XOR mask plus a class change when the window is drawn, lane-parallel
with LDS atomics, and a step of the top rung's wave is one row read.  Results are what they were: every case here is held bit for bit against the oracle's
scan = 3 -- the final state of every rung, class counts, samples, tops0 -- on shapes that cross windows, use every state width, an even lattice (no class
change), a top rung right above the bottom one, a ragged second workgroup, replicas, every p_logical regime, a run continued inside a window, and the
other three codes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _reference(orc, ocode, name, init, p, Nc, steps, p_logical, R, first, seed, tops_burn=1):
    """the oracle's ladders one by one (scan = 3): states, flags, counts, samples, tops0 per ladder"""
    M = init.shape[0] * R
    ncls = 16 if name == "toric" else 4
    counts = np.zeros((M, ncls), np.uint32); samples = np.zeros(M, np.uint64); tops0 = np.zeros(M, np.uint64)
    states = np.zeros((M, Nc) + init.shape[1:], np.uint8)
    for l in range(M):
        ld = orc.Ladder(ocode, init[l // R], p, Nc, p_logical, scan=3)
        r = orc.Rng.philox(seed, first + l)
        for _ in range(steps):
            ld.step(10, r)
            if ld.tops0 >= tops_burn:
                counts[l, orc.surf_eq_class(ocode, ld.states[0]) if name != "toric" else orc.toric_eq_class(ld.states[0])] += 1
                samples[l] += 1
        tops0[l] = ld.tops0
        states[l] = ld.states
    N = init.shape[0]
    return dict(states=states, counts=counts.reshape(N, R, ncls).sum(axis=1), samples=samples.reshape(N, R).sum(axis=1).astype(np.uint32),
                tops0=tops0.reshape(N, R).sum(axis=1).astype(np.uint32))


CASES = [  # name, L, Nc, N, steps, p, p_logical, replicas, first_syndrome
    ("toric", 9, 8, 6, 30, 0.15, 0.5, 1, 0), ("toric", 9, 8, 6, 30, 0.15, 1.0, 1, 0),          # the headline kernel: 12 words, two windows and a half
    ("toric", 9, 8, 6, 30, 0.15, 0.25, 1, 64), ("toric", 9, 8, 6, 30, 0.15, 0.0, 1, 0),        # ... no logical moves: stabilizers only
    ("toric", 4, 4, 5, 30, 0.12, 0.5, 1, 0),                                                   # even L: the operators leave the class alone; 2 of 4 words
    ("toric", 3, 2, 7, 40, 0.10, 0.5, 1, 0),                                                   # 4-word kernel, the top rung and one below it
    ("toric", 11, 8, 3, 30, 0.18, 0.5, 1, 0),                                                  # 16 words
    ("toric", 7, 5, 4, 30, 0.12, 0.5, 1, 0),                                                   # 7 of 8 words; five rungs: the cascade once per workgroup
    ("toric", 5, 5, 70, 30, 0.10, 0.5, 1, 128),                                                # two workgroups, the second ragged
    ("toric", 5, 4, 3, 30, 0.10, 0.5, 3, 64),                                                  # replicas
    ("xzzx", 9, 8, 4, 30, 0.15, 0.5, 1, 0), ("rotated", 7, 7, 4, 30, 0.17, 0.5, 1, 0), ("planar", 5, 5, 4, 30, 0.12, 0.5, 1, 0)]


@pytest.mark.parametrize("name,L,Nc,N,steps,p,p_logical,R,first", CASES)
def test_frames_bit_exact(q, orc, name, L, Nc, N, steps, p, p_logical, R, first):
    rng = np.random.default_rng(100 * L + 10 * Nc + N)
    code, ocode = _codes(q, orc, name)
    init = _init(rng, name, N, L, p)
    got = q.pteq_batch(init, p, Nc=Nc, code=code, scan="wave", p_logical=p_logical, return_states=True, replicas=R, steps=steps, iters=10, tops_burn=1,
                       seed=31, first_syndrome=first)
    ref = _reference(orc, ocode, name, init, p, Nc, steps, p_logical, R, first, 31)
    for key in ("states", "counts", "samples", "tops0"):
        assert np.array_equal(got[key], ref[key]), key


def test_a_run_continued_inside_a_window_is_the_one_long_run(q, orc):
    """7 steps, then 20: the second launch starts at step 7 of a window of 12 -- it builds the whole window and begins at its own row"""
    from qecmc.harness import LadderRun
    rng = np.random.default_rng(12)
    N, L, Nc, p = 6, 9, 8, 0.15
    init = _init(rng, "toric", N, L, p)
    run = LadderRun(init, p, Nc=Nc, iters=10, tops_burn=1, p_logical=0.5, seed=31, first_syndrome=64, scan="wave")
    got = run.advance(7).advance(20).snapshot(states=True)
    run.close()
    ref = _reference(orc, orc.TORIC, "toric", init, p, Nc, 27, 0.5, 1, 64, 31)
    for key in ("states", "counts", "samples", "tops0"):
        assert np.array_equal(got[key], ref[key]), key
