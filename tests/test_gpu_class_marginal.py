"""The exact per-qubit marginals on the GPU (qecmc_class_marginals, qecmc_class_marginals_site): the kernels' weights and z equal the host twin's --
the plain loops of csrc/class_marginal.hpp compiled by g++, which tests/test_class_marginal_cpu.py pins against the conditioning identity and a brute
force -- AS BYTES: both sides run the same single multiplies and adds in the order THE RULE of class_marginal.hpp writes down, the fold included.
The shapes are the smallest that reach each branch of the kernels: one lane group, cells that hold no qubit, more live states than lanes of a pass
and several terms per fold lane, held generators across a launch group, jobs across several workspace launches at toric L = 5 and the 128 KiB state
vector.  Then the weight vectors, the site form, dirty memory, the refusals -- and the purpose: the exact error count against 1 024 exact draws."""
import numpy as np
import pytest

import test_class_marginal_cpu as cpu
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape

pytestmark = pytest.mark.gpu

NAME = cpu.NAME
DEPOL, BIASED, WITH_ZERO = cpu.DEPOL, cpu.BIASED, cpu.WITH_ZERO


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return cpu.load_twin()


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([94, code, L, seed]))


def run_equal(q, T, code, L, n, w=None, wq=None, lds_width=0, seed=0, chains=None):
    """the GPU's dict against the twin's (weights, z, cls): as bytes"""
    chains = chains_of(code, L, n, seed) if chains is None else chains
    if wq is not None:
        table = np.asarray(wq).reshape(((len(wq),) if np.asarray(wq).ndim == 3 else ()) + state_shape(code, L) + (4,))
        got = q.class_marginals_site(NAME[code], chains, table, lds_width=lds_width, normalize=False)
    else:
        got = q.class_marginals(NAME[code], chains, w4=w, lds_width=lds_width, normalize=False)
    out, z, cls = cpu.twin(T, code, L, chains, w=w, wq=wq, lds_width=lds_width)
    assert got["weights"].dtype == np.float64 and got["z"].dtype == np.float64
    assert got["weights"].shape == out.shape[:2] + state_shape(code, L) + (4,)
    assert got["z"].tobytes() == z.tobytes()
    assert got["weights"].tobytes() == out.tobytes()
    assert np.array_equal(got["cls"], cls)
    return got


# ------------------------------------------------------------------------------------------------------ (1) the GPU is the twin, branch by branch
# (code, L, lds_width, N, the plan's (width, held))
BRANCHES = [(ROTATED, 3, 0, 3, (4, 0)),       # one lane group
            (PLANAR, 4, 0, 2, (8, 0)),        # cells that hold no qubit
            (ROTATED, 7, 0, 2, (10, 0)),      # more live states than lanes of a pass, 16 terms per fold lane
            (TORIC, 3, 6, 40, (6, 7)),        # held generators across the launch group of 32 syndromes
            (TORIC, 5, 13, 1, (13, 8)),       # the default route of the headline code: jobs across several workspace launches
            (ROTATED, 11, 0, 1, (14, 0))]     # the 128 KiB state vector


@pytest.mark.parametrize("code,L,lds_width,n,plan", BRANCHES)
def test_gpu_equals_host_twin(q, T, code, L, lds_width, n, plan):
    got = run_equal(q, T, code, L, n, w=DEPOL, lds_width=lds_width)
    assert (got["width"], got["held"]) == plan
    pn = cpu.plan_numbers(T, code, L, lds_width)
    assert (pn["width"], pn["held"]) == plan
    S, jobs = cpu.group_of(T, n, 16 if code == TORIC else 4, pn)
    if n == 40:
        assert S == 32 < n
        assert len({r.tobytes() for r in got["weights"]}) > 4                   # (many different syndromes: a row in the wrong place would show)
    if (code, L) == (TORIC, 5):
        assert jobs < (16 << plan[1])                                           # more than one workspace launch for the one syndrome
    if code == PLANAR:
        unused = ~cpu.qubit_cells(cpu.generators(code, L))
        assert unused.any() and (np.count_nonzero(got["weights"].reshape(n, 4, -1, 4)[:, :, unused], axis=-1) == 1).all()


@pytest.mark.parametrize("w", [DEPOL, BIASED, WITH_ZERO], ids=["depolarizing", "biased", "with-zero"])
def test_the_weight_vectors_at_rotated_L5(q, T, w):
    got = run_equal(q, T, ROTATED, 5, 4, w=w, seed=1)
    if w is WITH_ZERO:
        assert (got["weights"][..., 2] == 0.0).all()                            # a Pauli of weight 0: exact zeros


# ------------------------------------------------------------------------------------------------------ (3) the site form
@pytest.mark.parametrize("code,L,lds_width", [(XZZX, 5, 0), (TORIC, 3, 6)])
def test_site_tables(q, T, code, L, lds_width):
    n, nq = 3, int(np.prod(state_shape(code, L)))
    rng = np.random.default_rng([95, code])
    one, per = rng.uniform(0.05, 1.0, size=(nq, 4)), rng.uniform(0.05, 1.0, size=(n, nq, 4))
    run_equal(q, T, code, L, n, wq=one, lds_width=lds_width)
    run_equal(q, T, code, L, n, wq=per, lds_width=lds_width)
    const = run_equal(q, T, code, L, n, wq=np.broadcast_to(BIASED, (nq, 4)).copy(), lds_width=lds_width)
    uniform = run_equal(q, T, code, L, n, w=BIASED, lds_width=lds_width)
    assert const["weights"].tobytes() == uniform["weights"].tobytes() and const["z"].tobytes() == uniform["z"].tobytes()    # constant rows: the uniform entry point


def test_pure_erasure_is_exact(q, T):
    L = 3
    erased = np.zeros((L, L), bool)
    erased.ravel()[[0, 1, 2, 3, 4]] = True
    err = np.zeros((1, L, L), np.uint8)
    err[0][erased] = np.random.default_rng(2).integers(0, 4, size=int(erased.sum()))
    tab = q.erasure_site_w4([1.0, 0.0, 0.0, 0.0], erased)
    got = run_equal(q, T, ROTATED, L, 1, wq=tab.reshape(L * L, 4), chains=err)
    w, z = got["weights"][0], got["z"][0]
    assert (z > 0).any() and (z == 0).any() and (z == np.round(z)).all()        # counts of chains
    assert w[:, ~erased][..., 0].tobytes() == np.repeat(z[:, None], int((~erased).sum()), axis=1).tobytes() and (w[:, ~erased][..., 1:] == 0.0).all()
    assert (w[z == 0] == 0.0).all()
    with pytest.raises(FloatingPointError, match="row 0, class %d" % int(np.flatnonzero(z == 0)[0])):
        q.class_marginals_site("rotated", err, tab)
    post = q.posterior_marginals("rotated", err, site_weights=tab)
    assert (post[0][~erased][:, 0] == 1.0).all() and np.allclose(post.sum(axis=-1), 1.0)


# ------------------------------------------------------------------------------------------------------ (4) dirty memory
def test_dirty_workspace_and_dirty_lds_change_nothing(q, T):
    """0xFF bytes written, freed and handed back to the runtime, then the same call twice with a call of another shape and a shortest_chains call in
    between: the forward record, the partials, M_h and LDS come back dirty -- and the results are the same bytes"""
    import ctypes as C
    hip = q.lib()                                                               # (the handle resolves the HIP runtime the library is linked against)
    block, size = C.c_void_p(), 1 << 29
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t], [C.c_void_p]
    assert hip.hipMalloc(C.byref(block), size) == 0 and hip.hipMemset(block, 0xFF, size) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipFree(block) == 0
    first = run_equal(q, T, ROTATED, 7, 3, w=BIASED, seed=3)
    run_equal(q, T, TORIC, 3, 3, w=BIASED, lds_width=9, seed=3)                 # another shape, held generators, in the same blocks
    q.shortest_chains("rotated", chains_of(ROTATED, 7, 3, seed=4))              # integers in the same LDS
    again = run_equal(q, T, ROTATED, 7, 3, w=BIASED, seed=3)
    for k in ("weights", "z", "cls"):
        assert first[k].tobytes() == again[k].tobytes(), k


# ------------------------------------------------------------------------------------------------------ (5) refusals
def test_refusals_reach_the_caller(q):
    zero = np.zeros((2, 3, 3), np.uint8)
    zero[1, 0, 0] = 1
    with pytest.raises(FloatingPointError, match="row 0, class 1"):
        q.class_marginals("rotated", zero, w4=[1.0, 0.0, 0.0, 0.0])
    with pytest.raises(FloatingPointError, match="row 1"):
        q.posterior_marginals("rotated", zero, w4=[1.0, 0.0, 0.0, 0.0])         # row 1 has an X: no chain of any class is the identity everywhere
    with pytest.raises(FloatingPointError, match="row 0"):
        q.posterior_marginals("rotated", zero, w4=[1e300] * 4)
    with pytest.raises(q.QecmcError, match="qecmc_class_marginals: w\\[1\\]=-1"):
        q.class_marginals("rotated", zero, w4=[1.0, -1.0, 0.0, 0.0])
    with pytest.raises(q.QecmcError, match="qecmc_class_marginals_site: lds_width=15"):
        q.class_marginals_site("rotated", zero, np.ones((3, 3, 4)), lds_width=15)
    raw = q.class_marginals("rotated", zero, w4=[1.0, 0.0, 0.0, 0.0], normalize=False)
    assert raw["z"][0].tolist() == [1.0, 0.0, 0.0, 0.0] and "marginals" not in raw


# ------------------------------------------------------------------------------------------------------ (6) the purpose: the exact count against draws
@pytest.mark.parametrize("code,L", [(TORIC, 3), (ROTATED, 7)])
def test_exact_error_count_against_exact_draws(q, code, L):
    """per syndrome |exact - mean of 1 024 draws| <= 5 std / sqrt(1024), the std taken from the draws; fixed seed (the twins stay inside:
    tests/test_class_marginal_cpu.py::test_exact_count_against_the_samplers_twin)"""
    m, p, K = cpu.dense_errors(code, L, 8), 0.1, 1024
    exact = q.exact_error_counts(NAME[code], m, p)
    mean = q.posterior_error_counts(NAME[code], m, p, K, seed=cpu.SA.SEED)
    draws = q.sample_posterior(NAME[code], m, p=p, n_samples=K, seed=cpu.SA.SEED)["chains"]
    n_err = (draws.reshape(8, K, -1) != 0).sum(axis=2)
    assert np.array_equal(n_err.mean(axis=1), mean)
    bar = n_err.std(axis=1, ddof=1) / np.sqrt(K)
    print("exact", exact["posterior"], "draws", mean, "|d| / bar", np.abs(exact["posterior"] - mean) / bar)
    assert (bar > 0).all() and (np.abs(exact["posterior"] - mean) <= 5.0 * bar).all()
    z = q.class_sweep_cut(NAME[code], m, q.depolarizing_w4(p))["Z"]
    assert np.allclose(exact["posterior"], (exact["per_class"] * z).sum(axis=1) / z.sum(axis=1), rtol=1e-12)
