"""scan = "wave", who draws the swap uniforms (csrc/ladder_wu.hpp, the lean step tail): in the kernels of up to 8 rungs whose top role is the frame role
(fixed length, up to 16 state words, iters = 10) the top rung's wave draws both blocks of four such a ladder has and the waves below it draw none; the
kernels of 9 to 16 rungs keep one block per wave, the top four.  The words are addressed by (step, block, ladder), so nothing a run returns may move: every case is held bit for bit against the
oracle's scan = 3 -- counts, samples, tops0, the final state and the flag of every rung -- over 30 steps (two pick windows and a half) at the ladder
lengths where the blocks begin and end (2, 5, 6, 8, 9, 10, 12, 16 rungs), on several workgroups with a ragged last one, with and without logical moves, in
a run continued at step 7 of a window, and on one xzzx lattice."""
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


def _init(rng, name, N, L, p):
    shape = (N, 2, L, L) if name == "toric" else (N, L, L)
    return (rng.integers(1, 4, size=shape) * (rng.random(shape) < p)).astype(np.uint8)


def _reference(orc, name, init, p, Nc, steps, p_logical, first, seed):
    """the oracle's ladders one by one (scan = 3): states, flags, counts, samples, tops0 per ladder (tops_burn = 1)"""
    ocode = orc.TORIC if name == "toric" else orc.XZZX
    N = init.shape[0]
    ncls = 16 if name == "toric" else 4
    counts = np.zeros((N, ncls), np.uint32); samples = np.zeros(N, np.uint32); tops0 = np.zeros(N, np.uint32)
    states = np.zeros((N, Nc) + init.shape[1:], np.uint8); flags = np.zeros((N, Nc), np.uint8)
    for l in range(N):
        ld = orc.Ladder(ocode, init[l], p, Nc, p_logical, scan=3)
        r = orc.Rng.philox(seed, first + l)
        for _ in range(steps):
            ld.step(10, r)
            if ld.tops0 >= 1:
                counts[l, orc.toric_eq_class(ld.states[0]) if name == "toric" else orc.surf_eq_class(ocode, ld.states[0])] += 1
                samples[l] += 1
        tops0[l] = ld.tops0; states[l] = ld.states; flags[l] = ld.flags
    return dict(states=states, flags=flags, counts=counts, samples=samples, tops0=tops0)


STEPS = 30
CASES = [  # name, L, Nc, N, p, p_logical, first_syndrome, chunks
    ("toric", 3, 8, 134, 0.10, 0.5, 0, (30,)),       # the 4-word kernel at the headline's length: three workgroups, the last one ragged
    ("toric", 5, 8, 70, 0.12, 0.0, 64, (30,)),       # no logical moves; a ragged second workgroup
    ("toric", 5, 8, 70, 0.12, 0.5, 64, (7, 23)),     # continued at step 7 of a window
    ("toric", 3, 2, 5, 0.10, 0.5, 0, (30,)),         # one pair
    ("toric", 3, 5, 5, 0.10, 0.5, 0, (30,)),         # four pairs: block 0 alone, full
    ("toric", 5, 6, 6, 0.12, 0.5, 0, (30,)),         # five pairs: one word of block 1
    ("toric", 5, 9, 4, 0.12, 0.5, 0, (30,)),         # eight pairs: blocks 0 and 1 full, none below the top (1 024 threads)
    ("toric", 5, 10, 4, 0.12, 0.5, 0, (30,)),        # nine pairs: one word of block 2, drawn two rungs below the top
    ("toric", 5, 12, 4, 0.12, 0.5, 64, (30,)),       # eleven pairs
    ("toric", 3, 16, 66, 0.10, 0.5, 0, (30,)),       # fifteen pairs: all four blocks; ragged
    ("xzzx", 5, 8, 6, 0.12, 0.5, 0, (30,)),
]


@pytest.mark.parametrize("name,L,Nc,N,p,p_logical,first,chunks", CASES)
def test_swap_uniforms_drawn_by_the_top_role_bit_exact(q, orc, name, L, Nc, N, p, p_logical, first, chunks):
    from qecmc.harness import LadderRun
    rng = np.random.default_rng(1000 * L + 10 * Nc + N)
    init = _init(rng, name, N, L, p)
    run = LadderRun(init, p, Nc=Nc, iters=10, tops_burn=1, p_logical=p_logical, seed=57, first_syndrome=first, scan="wave",
                    code=q.TORIC if name == "toric" else q.XZZX)
    for c in chunks:
        run.advance(c)
    got = run.snapshot(states=True)
    run.close()
    assert sum(chunks) == STEPS
    ref = _reference(orc, name, init, p, Nc, STEPS, p_logical, first, 57)
    for key in ("states", "flags", "counts", "samples", "tops0"):
        assert np.array_equal(got[key], ref[key]), key
