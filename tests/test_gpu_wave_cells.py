"""The toric scan = "wave" kernels on the wave layout (csrc/ladder_wu.hpp wu_read_cell / wu_xor_cell, csrc/tables.hpp toric_wave_descriptors): the two
layers interleaved in the state words, a generator's own cell read and updated through one word.  The layout is internal to the kernels -- inputs,
final states and the resume format stay byte-per-qubit in the reference's order --, so every shape is compared bit for bit with the oracle's
scan = 3: class counts, samples, tops0 and every rung's final configuration, with logical moves on (p_logical = 0.5) and every step recorded
(tops_burn = 0).  The shapes are the ones at which the layout can go wrong: a partial last word, a last word of one cell, even L, every state
width's kernel family member that a toric lattice reaches cheaply (4, 12, 32 words; fixed length, criterion, queue), staging and write-out through
the byte format in the middle of a run."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, SEED = 0.12, 41


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


def _init(L, N):
    rng = np.random.default_rng(100 * L + N)
    shape = (N, 2, L, L)
    return (rng.integers(1, 4, size=shape) * (rng.random(shape) < P)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _reference(L, Nc, N, steps, iters, first):
    """the oracle's run of a fixed-length case: computed once, shared by the tests that need it"""
    from oracle import oracle as orc
    ref = orc.pteq_batch(orc.TORIC, _init(L, N), P, Nc, steps, iters=iters, tops_burn=0, seed=SEED, first_syndrome=first, return_states=True, scan=3)      # (p_logical = 0.5: the oracle's batch drivers run decoders.py's default)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _same(got, ref):
    assert np.array_equal(got["states"], ref["states"])
    assert np.array_equal(got["counts"], ref["counts"])
    assert np.array_equal(got["samples"], ref["samples"].astype(np.uint32))
    assert np.array_equal(got["tops0"], ref["tops0"].astype(np.uint32))


FIXED = [  # L, Nc, N, steps, iters, first_syndrome
    (3, 2, 70, 100, 10, 0),        # two words, the last one partial (one cell); two workgroups, the second ragged
    (4, 3, 5, 150, 3, 64),         # even L: two full words; the general proposal loop
    (5, 5, 70, 100, 10, 128),      # the cascade once per workgroup; cell 24 alone in the fourth word
    (9, 8, 128, 30, 10, 0),        # the headline instantiation: 11 of 12 words, the last one holding one cell
    (12, 4, 64, 20, 10, 64)]       # the 32-word kernel: 18 words, the exchange in two halves


@pytest.mark.parametrize("L,Nc,N,steps,iters,first", FIXED)
def test_wave_cells_bit_exact(q, L, Nc, N, steps, iters, first):
    got = q.pteq_batch(_init(L, N), P, Nc=Nc, steps=steps, iters=iters, tops_burn=0, seed=SEED, p_logical=0.5, first_syndrome=first, return_states=True, scan="wave")
    ref = _reference(L, Nc, N, steps, iters, first)
    _same(got, ref)
    assert not np.array_equal(ref["states"][:, 0], _init(L, N)) and ref["counts"].sum() == N * steps      # (the run moved, every step was recorded)


def test_wave_cells_two_resumed_launches_equal_one(q):
    """L = 9, Nc = 8: two launches of 15 steps through qecmc_pteq_resume_dev -- the state leaves the kernel and re-enters it through the byte format --
    equal the one launch of 30"""
    import torch
    from qecmc import _lib as L_
    L, Nc, N, steps, iters, first = FIXED[3]
    init = _init(L, N)
    nq = 2 * L * L
    dev = torch.device("cuda", 0)
    states = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(init.reshape(N, 1, nq), (N, Nc, nq)))).to(dev)
    fl = np.zeros((N, Nc), dtype=np.uint8); fl[:, -1] = 1
    flg = torch.from_numpy(fl).to(dev)
    tops0 = torch.zeros(N, dtype=torch.int32, device=dev)
    counts = torch.zeros((N, 16), dtype=torch.int32, device=dev)
    samples = torch.zeros(N, dtype=torch.int32, device=dev)
    done = 0
    for chunk in (15, 15):
        pl = C.c_void_p()
        pr = L_.make_params(code=L_.TORIC, L=L, Nc=Nc, p=P, p_logical=0.5, iters=iters, steps=chunk, tops_burn=0, seed=SEED, scan=L_.SCAN_WAVE)
        L_.check(L_.lib().qecmc_plan_create(pr, C.byref(pl)))
        try:
            L_.check(L_.lib().qecmc_pteq_resume_dev(pl, states.data_ptr(), flg.data_ptr(), tops0.data_ptr(), N, first, done, counts.data_ptr(),
                                                    samples.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            torch.cuda.synchronize()
        finally:
            L_.lib().qecmc_plan_destroy(pl)
        done += chunk
    assert done == steps
    got = dict(states=states.cpu().numpy().reshape((N, Nc, 2, L, L)), counts=counts.cpu().numpy().view(np.uint32),
               samples=samples.cpu().numpy().view(np.uint32), tops0=tops0.cpu().numpy().view(np.uint32))
    _same(got, _reference(L, Nc, N, steps, iters, first))


CRIT = dict(iters=10, tops_burn=0, seed=SEED, SEQ=2, TOPS=4, eps=0.3)


def _same_criterion(got, ref):
    for k in ("counts", "samples", "tops0", "steps_done"):
        assert np.array_equal(got[k], ref[k].astype(got[k].dtype)), k
    assert np.array_equal(got["converged"], ref["converged"])


def test_wave_cells_criterion_bit_exact(q):
    """L = 5, Nc = 5 with the error_based criterion, one ladder per lane (the criterion kernels keep the exchange buffer's tight rows)"""
    from oracle import oracle as orc
    L, Nc, N, steps = 5, 5, 70, 4000
    init = _init(L, N)
    got = q.pteq_batch(init, P, Nc=Nc, scan="wave", steps=steps, first_syndrome=64, conv_criteria="error_based", p_logical=0.5, **CRIT)
    ref = orc.pteq_batch(orc.TORIC, init, P, Nc, steps, scan=3, first_syndrome=64, conv_criteria="error_based", **CRIT)
    assert ref["converged"].any()
    _same_criterion(got, ref)


def test_wave_cells_work_queue_bit_exact(q):
    """... and on the persistent grid, forced down to two workgroups: every lane stages several ladders in the middle of the run"""
    from oracle import oracle as orc
    L, Nc, N, steps, grid = 5, 5, 400, 3000, 2
    init = _init(L, N)
    got = q.pteq_batch(init, P, Nc=Nc, scan="wave", steps=steps, first_syndrome=128, conv_criteria="error_based", flags=q.dev_flags(queue_grid=grid), p_logical=0.5, **CRIT)
    ref = orc.pteq_wave_queue(orc.TORIC, init, P, Nc, steps, grid, first_syndrome=128, **CRIT)
    assert ref["converged"].any() and not ref["converged"].all()
    _same_criterion(got, ref)
