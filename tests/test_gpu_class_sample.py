"""The exact chain sampler on the GPU (qecmc_class_sample, qecmc_class_sample_site): the kernels' chains, classes and z equal the host twin's -- the
plain loops of csrc/class_sample.hpp compiled by g++, which tests/test_class_sample_cpu.py pins against the oracle and a brute-force law -- BYTE FOR
BYTE, z as bits: both sides run the same single multiplies, adds and compares on the same Philox words.  The shapes are the smallest that reach each
branch of the kernels: one lane group, more samples than a wave, more live states than lanes of a FORGET pass, held generators with a job per sample
across a launch group, the default route at toric L = 5 and the 128 KiB state vector.  Then the weight vectors, the site form, dirty memory -- and
the purpose of it all: the samplers' rung-0 error counts against exact draws at the headline shape.

The purpose test's figures, measured on an MI355X (mean d, std(d) / sqrt(64), |mean d| in units of that error bar), are in DESIGN.md 4.1s."""
import numpy as np
import pytest

import test_class_sample_cpu as cpu
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape

pytestmark = pytest.mark.gpu

NAME = cpu.NAME
DEPOL, BIASED, WITH_ZERO = cpu.DEPOL, cpu.BIASED, cpu.WITH_ZERO
SEED = cpu.SEED


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return cpu.load_twin()


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([83, code, L, seed]))


def run_equal(q, T, code, L, n, K, mode, w=None, wq=None, lds_width=0, seed=0, first=0, chains=None):
    """the GPU's dict against the twin's (chains, cls, z): bytes, and z as bits"""
    chains = chains_of(code, L, n, seed) if chains is None else chains
    kw = dict(n_samples=K, seed=SEED, first_syndrome=first, lds_width=lds_width)
    if wq is not None:
        table = np.asarray(wq).reshape(((len(wq),) if np.asarray(wq).ndim == 3 else ()) + state_shape(code, L) + (4,))
        got = q.sample_posterior(NAME[code], chains, site_weights=table, **kw) if mode else q.sample_chains_site(NAME[code], chains, table, **kw)
    else:
        got = q.sample_posterior(NAME[code], chains, w4=w, **kw) if mode else q.sample_chains(NAME[code], chains, w4=w, **kw)
    out, cls, z = cpu.twin(T, code, L, chains, w=w, wq=wq, K=K, first=first, mode=mode, lds_width=lds_width)
    assert got["chains"].dtype == np.uint8 and got["z"].dtype == np.float64
    assert got["chains"].shape == out.shape[:-1] + state_shape(code, L)
    assert got["z"].tobytes() == z.tobytes()
    assert np.array_equal(got["chains"].reshape(out.shape), out)
    if mode:
        assert got["cls"].dtype == np.int32 and np.array_equal(got["cls"], cls)
    return got


# ------------------------------------------------------------------------------------------------------ (a) the GPU is the twin, branch by branch
# (code, L, lds_width, N, K, the plan's (width, held))
BRANCHES = [(ROTATED, 3, 0, 3, 5, (4, 0)),       # one lane group
            (XZZX, 5, 0, 2, 70, (8, 0)),         # more samples than a wave
            (PLANAR, 4, 0, 2, 70, (8, 0)),       # more samples than a wave; cells that hold no qubit
            (ROTATED, 7, 0, 2, 3, (10, 0)),      # more live states than lanes of a FORGET pass: 512 against 256
            (TORIC, 3, 6, 40, 2, (6, 7)),        # held generators, a job per sample, across the launch group of 32 syndromes
            (TORIC, 5, 13, 1, 2, (13, 8)),       # the default route of the headline code
            (ROTATED, 11, 0, 1, 2, (14, 0))]     # the 128 KiB state vector


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("code,L,lds_width,n,K,plan", BRANCHES)
def test_gpu_equals_host_twin(q, T, code, L, lds_width, n, K, plan, mode):
    got = run_equal(q, T, code, L, n, K, mode, w=DEPOL, lds_width=lds_width)
    assert (got["width"], got["held"]) == plan
    if n == 40:
        g = np.zeros(3, np.uint32)
        T.qt_class_sample_group(n, 16, plan[1], K, cpu.plan_numbers(T, code, L, lds_width)["job_bytes"], g.ctypes.data_as(cpu._u32p))
        assert int(g[0]) == 32 < n
        assert len({r.tobytes() for r in got["chains"]}) > 4                    # (many different syndromes: a row in the wrong place would show)


@pytest.mark.parametrize("w,mode", [(DEPOL, 0), (BIASED, 0), (BIASED, 1), (WITH_ZERO, 1)])
def test_the_weight_vectors_at_rotated_L5(q, T, w, mode):
    got = run_equal(q, T, ROTATED, 5, 4, 9, mode, w=w, seed=1, first=1000)
    if w is WITH_ZERO:
        assert not (got["chains"] == 2).any()                                   # a Pauli of weight 0 is never drawn


def test_first_syndrome_and_seed_reach_the_kernels(q, T):
    chains = chains_of(XZZX, 5, 3, seed=2)
    a = run_equal(q, T, XZZX, 5, 3, 4, 0, w=DEPOL, chains=chains, first=(1 << 32) - 3)
    b = run_equal(q, T, XZZX, 5, 3, 4, 0, w=DEPOL, chains=chains, first=0)
    assert not np.array_equal(a["chains"], b["chains"])
    c = q.sample_chains("xzzx", chains[1:2], w4=DEPOL, n_samples=2, seed=SEED, first_syndrome=1)
    assert np.array_equal(c["chains"], b["chains"][1:2, :, :2])                 # sample (s, c, k) whatever N and K


# ------------------------------------------------------------------------------------------------------ (b) the site form
@pytest.mark.parametrize("code,L,lds_width", [(XZZX, 5, 0), (TORIC, 3, 6)])
def test_site_tables(q, T, code, L, lds_width):
    n, nq = 3, int(np.prod(state_shape(code, L)))
    rng = np.random.default_rng([84, code])
    one, per = rng.uniform(0.05, 1.0, size=(nq, 4)), rng.uniform(0.05, 1.0, size=(n, nq, 4))
    for mode in (0, 1):
        run_equal(q, T, code, L, n, 3, mode, wq=one, lds_width=lds_width)
        run_equal(q, T, code, L, n, 3, mode, wq=per, lds_width=lds_width)
        const = run_equal(q, T, code, L, n, 3, mode, wq=np.broadcast_to(BIASED, (nq, 4)).copy(), lds_width=lds_width)
        uniform = run_equal(q, T, code, L, n, 3, mode, w=BIASED, lds_width=lds_width)
        assert np.array_equal(const["chains"], uniform["chains"]) and const["z"].tobytes() == uniform["z"].tobytes()    # constant rows: the uniform entry point


def test_refusals_reach_the_caller(q):
    zero = np.zeros((2, 3, 3), np.uint8)
    zero[1, 0, 0] = 1
    with pytest.raises(q.QecmcError, match="qecmc_class_sample: row 0, class 1"):
        q.sample_chains("rotated", zero, w4=[1.0, 0.0, 0.0, 0.0])
    with pytest.raises(q.QecmcError, match="qecmc_class_sample: row 1: the class weights total 0"):
        q.sample_posterior("rotated", zero, w4=[1.0, 0.0, 0.0, 0.0])
    with pytest.raises(q.QecmcError, match="qecmc_class_sample: row 0.*inf"):
        q.sample_posterior("rotated", zero, w4=[1e300] * 4)


# ------------------------------------------------------------------------------------------------------ (c) dirty memory
def test_dirty_workspace_and_dirty_lds_change_nothing(q, T):
    """0xFF bytes written, freed and handed back to the runtime, then the same call twice with a call of another shape in between: the record, the
    partials, the job tables and LDS come back dirty -- the workspace recycled from another shape -- and the results are the same"""
    import ctypes as C
    hip = q.lib()                                                               # (the handle resolves the HIP runtime the library is linked against)
    block, size = C.c_void_p(), 1 << 29
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t], [C.c_void_p]
    assert hip.hipMalloc(C.byref(block), size) == 0 and hip.hipMemset(block, 0xFF, size) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipFree(block) == 0
    first = run_equal(q, T, ROTATED, 7, 3, 4, 1, w=BIASED, seed=3)
    run_equal(q, T, TORIC, 3, 3, 4, 0, w=BIASED, lds_width=9, seed=3)           # another shape, held generators, in the same blocks
    q.shortest_chains("rotated", chains_of(ROTATED, 7, 3, seed=4))              # integers in the same LDS
    again = run_equal(q, T, ROTATED, 7, 3, 4, 1, w=BIASED, seed=3)
    for k in ("chains", "cls", "z"):
        assert np.array_equal(first[k], again[k]), k


# ------------------------------------------------------------------------------------------------------ (d) the purpose: samplers against exact draws
@pytest.fixture(scope="module")
def headline(q):
    """toric L = 5, p = 0.1, 64 syndromes: the errors, and the exact posterior's mean error count per syndrome from 1 024 draws each -- computed once"""
    L, p, n = 5, 0.1, 64
    rng = np.random.default_rng(85)
    err = np.zeros((n, 2, L, L), np.uint8)
    hit = rng.random(err.shape) < p
    err[hit] = rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)
    return err, p, q.posterior_error_counts("toric", err, p, 1024, seed=SEED)


@pytest.mark.parametrize("scan", ["random", "wave"])
def test_rung_0_error_counts_against_exact_draws(q, headline, scan):
    """Per syndrome, rung 0's mean error count over 20 000 ladder steps after a burn-in -- nerr_sums of a run of burn + 20 000 steps minus nerr_sums of
    the same run stopped at burn: the chain is a function of its seed -- against the mean of 1 024 exact draws.  The differences d_s are paired by
    syndrome; |mean d| < 5 std(d) / sqrt(64): the error bar comes from the data"""
    err, p, exact = headline
    steps, burn = 20000, 2000
    kw = dict(Nc=5, iters=10, tops_burn=0, code=q.TORIC, scan=scan, return_swap_stats=True, seed=77)
    a = q.pteq_batch(err, p, steps=burn, **kw)
    b = q.pteq_batch(err, p, steps=burn + steps, **kw)
    mcmc = (b["nerr_sums"][:, 0].astype(np.int64) - a["nerr_sums"][:, 0]) / steps
    d = mcmc - exact
    bar = d.std(ddof=1) / np.sqrt(len(d))
    print("scan=%s: mean error count exact %.4f, sampler %.4f; mean d %.5f, std(d) / sqrt(64) %.5f, |mean d| / bar %.2f" %
          (scan, exact.mean(), mcmc.mean(), d.mean(), bar, abs(d.mean()) / bar))
    assert abs(d.mean()) < 5.0 * bar
