"""The exact chain sampler (csrc/class_sample.hpp), without a GPU: the twin, compiled by g++ into the host-table test library (qt_class_sample,
qt_class_sample_plan, qt_class_sample_group, qt_class_sample_u53), and the Python layer around it.

What is pinned: every sample has the input's syndrome and lies in its class, by the oracle; z is the cut twin's, bit for bit; THE LAW -- the counts
of 2^16 samples per class against the brute force of tests/util_class_sample.py by Pearson's chi-square, and the posterior's class counts against
Z_c / Z --; the same law where generators are held; a sample as a function of its address (seed, syndrome, class, k) alone; the low-p limit
against the (min, +) family; site tables, erasures; every refusal by name; the plan's numbers.  (The sanitizers: tests/test_class_sample_resources.py.)

The chi-square bound is the 1 - 1e-6 quantile of the distribution (util_class_sample.chi_square_quantile, exact).  Bins are pooled, smallest
probability first, until every bin expects 5 samples (Cochran's rule: below that Pearson's statistic does not follow the chi-square law) -- a rule on
the brute force's probabilities alone.  The runs are deterministic under SEED: the twin is checked to stay within the bound, once and for all."""
import ctypes as C

import numpy as np
import pytest

import test_class_minplus_trace_cpu as MT
import test_class_sweep_cut_cpu as SC
import test_class_sweep_site_cpu as SS
import util_class_sample as U
from qecmc import _lib as L_
from qecmc import exact as ex
from test_corrections_cpu import classes, generators, syndromes
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_minplus_trace import qubit_cells

NAME = MT.NAME
SEED = 20261020
WORKSPACE = 512 << 20
LAUNCH_SAMPLES = 1 << 18
_u8p, _u32p, _i32p, _u64p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
DEPOL = ex.depolarizing_w4(0.1)
BIASED = ex.biased_w4(0.1, 10.0)
WITH_ZERO = np.array([1.0, 0.3, 0.0, 0.2])
FLAT = np.array([1.0, 0.55, 0.4, 0.7])          # weights under which the 4 096 chains of a planar class all expect more than a sample in 2^16


def load_twin():
    """the host-table test library with the sampler's entry points (tests/test_gpu_class_sample.py compares the GPU with it)"""
    lib = SS.load_twin()
    MT.load_twin()
    lib.qt_class_sample.restype = C.c_int
    lib.qt_class_sample.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _f64p, _f64p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, _u8p, _i32p, _f64p,
                                    C.c_char_p, C.c_int]
    lib.qt_class_sample_plan.restype = C.c_int
    lib.qt_class_sample_plan.argtypes = [C.c_int, C.c_int, C.c_int, _i32p, _u32p, C.c_int, _u64p]
    lib.qt_class_sample_group.restype = None
    lib.qt_class_sample_group.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _u32p]
    lib.qt_class_sample_u53.restype = C.c_double
    lib.qt_class_sample_u53.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def twin_rc(T, code, L, chains, w=None, wq=None, K=1, seed=SEED, first=0, mode=0, lds_width=0):
    """(rc, message, chains uint8[N, ncls, K, nq] or [N, K, nq], cls int32[N, K], z float64[N, ncls]) of the host twin; the outputs start out poisoned.
    wq: float[rows, nq, 4] or [nq, 4]"""
    nq = int(np.prod(state_shape(code, L))) if 2 <= L <= 64 else 1
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    n, ncls = len(flat), 16 if code == TORIC else 4
    kk = K if 0 < K < 1 << 20 else 1
    out = np.full((n, kk, nq) if mode == 1 else (n, ncls, kk, nq), 0xEE, np.uint8)
    cls, z = np.full((n, kk), 99, np.int32), np.full((n, ncls), -1.0)
    msg = C.create_string_buffer(640)
    wp = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    tab = None if wq is None else np.ascontiguousarray(wq, dtype=np.float64).reshape(-1, nq, 4)
    rc = T.qt_class_sample(code, L, n, flat.ctypes.data_as(_u8p), None if wp is None else wp.ctypes.data_as(_f64p), None if tab is None else tab.ctypes.data_as(_f64p),
                           0 if tab is None else len(tab), lds_width, K, seed, first, mode, out.ctypes.data_as(_u8p), cls.ctypes.data_as(_i32p), z.ctypes.data_as(_f64p), msg, 640)
    return rc, msg.value.decode(), out, cls, z


def twin(T, code, L, chains, **kw):
    rc, msg, out, cls, z = twin_rc(T, code, L, chains, **kw)
    assert rc == 0, msg
    return out, cls, z


def plan_numbers(T, code, L, lds_width):
    out6 = np.zeros(6, np.uint64)
    n = T.qt_class_sample_plan(code, L, lds_width, None, None, 0, out6.ctypes.data_as(_u64p))
    assert n >= 0
    return dict(zip(("n_forget", "W", "width", "held", "workspace", "job_bytes"), (int(x) for x in out6)))


def errors(code, L, n, seed):
    return random_errors(code, L, n, np.random.default_rng(seed))


# ------------------------------------------------------------------------------------------------------ the plan's numbers
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 3, 0), (ROTATED, 9, 0), (ROTATED, 11, 0), (PLANAR, 7, 0), (TORIC, 3, 6), (TORIC, 5, 13), (TORIC, 5, 14)])
def test_record_bytes_and_launch_group(T, code, L, lds_width):
    _, inf, _ = SC.info(T, code, L, lds_width)
    pn = plan_numbers(T, code, L, lds_width)
    print(NAME[code], L, lds_width, pn)
    assert pn["n_forget"] == inf["n_gen"] - inf["held"] and pn["width"] == inf["width"] and pn["held"] == inf["held"] and pn["workspace"] == WORKSPACE
    assert pn["job_bytes"] == pn["n_forget"] * (1 << (inf["width"] - 1)) * 16
    assert MT.trace_plan(T, code, L, lds_width)[2]["n_forget"] == pn["n_forget"]                  # the FORGETs are the traceback's
    g = np.zeros(3, np.uint32)
    for n in (1, 2, 40, 5000, 1 << 32):
        for K in (1, 70, 1024, (1 << 32) - 1):
            T.qt_class_sample_group(n, inf["ncls"], inf["held"], K, pn["job_bytes"], g.ctypes.data_as(_u32p))
            S, kc, jobs = (int(x) for x in g)
            assert 1 <= S <= T.qt_class_sweep_cut_group(n, inf["ncls"], inf["held"]) and 1 <= kc <= K and jobs >= 1
            assert jobs * pn["job_bytes"] <= WORKSPACE                          # the records of one launch
            assert S * inf["ncls"] * kc <= LAUNCH_SAMPLES                       # the samples of one launch
            if inf["held"] == 0:
                assert jobs == S * inf["ncls"]                                  # every pair of the group has its record at once


def test_uniform_is_the_documented_address(T):
    for seed, syn, stream, k, block, j in [(0, 0, 0, 0, 0, 0), (SEED, 7, 3, 5, 1, 1), ((1 << 63) + 5, (1 << 32) - 1, 16, (1 << 32) - 1, 122, 0), (9, 1 << 31, 4, 1 << 20, 60, 1)]:
        u = T.qt_class_sample_u53(k, block, j, syn, stream, seed)
        assert u == U.u53(seed, syn, stream, k, block, j) and 0.0 <= u < 1.0
    base = (SEED, 7, 3, 5, 1, 1)
    for i in range(6):                                                          # changing any one of seed, s, c, k (and block, j) changes the draw
        other = list(base)
        other[i] = base[i] + 1 if i != 5 else 0
        assert U.u53(*other) != U.u53(*base)


# ------------------------------------------------------------------------------------------------------ syndrome, class, z
@pytest.mark.parametrize("code,L", [(TORIC, 3), (XZZX, 3), (ROTATED, 3), (PLANAR, 3), (ROTATED, 5), (XZZX, 5), (ROTATED, 7), (XZZX, 7)])
def test_samples_keep_the_syndrome_and_lie_in_their_class(T, code, L):
    m = errors(code, L, 3, 100 + L)
    want_syn, ncls = syndromes(code, m), 16 if code == TORIC else 4
    z_cut, _ = SC.twin(T, code, L, m, DEPOL)
    out, _, z = twin(T, code, L, m, w=DEPOL, K=4)
    assert z.tobytes() == z_cut.tobytes()                                       # bit for bit the cut twin's
    for s in range(3):
        for c in range(ncls):
            got = out[s, c].reshape((4,) + state_shape(code, L))
            assert np.array_equal(syndromes(code, got), np.broadcast_to(want_syn[s], (4,) + want_syn[s].shape)) and (classes(code, got) == c).all()
    post, cls, z1 = twin(T, code, L, m, w=DEPOL, K=4, mode=1)
    assert z1.tobytes() == z_cut.tobytes() and ((0 <= cls) & (cls < ncls)).all()
    for s in range(3):
        got = post[s].reshape((4,) + state_shape(code, L))
        assert np.array_equal(classes(code, got), cls[s]) and np.array_equal(syndromes(code, got), np.broadcast_to(want_syn[s], (4,) + want_syn[s].shape))
        assert all(np.array_equal(post[s, k], out[s, cls[s, k], k]) for k in range(4))        # posterior[s, k] == every_class[s, cls[s, k], k]


# ------------------------------------------------------------------------------------------------------ the law
def check_law(counts, prob, what):
    stat, dof = U.chi_square(counts, prob)
    if dof <= 0:                                                                # one bin: every sample is in it
        assert stat == 0.0, what
        return
    bound = U.chi_square_quantile(dof)
    print("%s: chi-square %.1f over %d degrees of freedom, bound %.1f" % (what, stat, dof, bound))
    assert stat <= bound, what


@pytest.mark.parametrize("code,w", [(ROTATED, DEPOL), (XZZX, BIASED), (PLANAR, FLAT)])
def test_the_law_of_every_class_against_the_brute_force(T, code, w):
    K = 1 << 16
    m = errors(code, 3, 2, 7)
    out, _, z = twin(T, code, 3, m, w=w, K=K)
    post_cls = twin(T, code, 3, m, w=w, K=K, mode=1)[1]
    for s in range(2):
        law = U.class_law(code, 3, m[s], w)
        for c, (chains, prob, zc) in enumerate(law):
            assert len(chains) == (4096 if code == PLANAR else 256) and abs(z[s, c] - zc) <= 1e-12 * zc
            check_law(U.counts_of(out[s, c], chains), prob, "%s syndrome %d class %d" % (NAME[code], s, c))
        zs = np.array([zc for _, _, zc in law])
        check_law(np.bincount(post_cls[s], minlength=4), zs / zs.sum(), "%s syndrome %d: the posterior's classes" % (NAME[code], s))


@pytest.mark.parametrize("lds_width", [6, 7])
def test_the_law_with_held_generators(T, lds_width):
    """toric L = 3: 2^16 chains per class, binned by error count"""
    K = 4096
    assert SC.info(T, TORIC, 3, lds_width)[1]["held"] > 0
    m = errors(TORIC, 3, 1, 11)
    out, _, z = twin(T, TORIC, 3, m, w=FLAT, K=K, lds_width=lds_width)
    assert z.tobytes() == SC.twin(T, TORIC, 3, m, FLAT, lds_width)[0].tobytes()
    law = U.class_law(TORIC, 3, m[0], FLAT)
    for c, (chains, prob, _) in enumerate(law):
        assert len(chains) == 1 << 16
        n_err = np.count_nonzero(chains, axis=1)
        want = np.bincount(n_err, weights=prob, minlength=19)
        got = out[0, c]
        assert np.array_equal(syndromes(TORIC, got.reshape(-1, 2, 3, 3)), np.broadcast_to(syndromes(TORIC, m)[0], (K,) + syndromes(TORIC, m)[0].shape))
        assert (classes(TORIC, got.reshape(-1, 2, 3, 3)) == c).all()
        check_law(np.bincount(np.count_nonzero(got, axis=1), minlength=19), want, "toric width %d class %d by error count" % (lds_width, c))
    # ... and the X / Y / Z split, which the error count does not see: per class the number of Z over all samples against its expectation, 6 sigma
    for c, (chains, prob, _) in enumerate(law):
        nz = (chains == 3).sum(axis=1)
        mean, var = float((prob * nz).sum()), float((prob * nz * nz).sum() - (prob * nz).sum() ** 2)
        assert abs((out[0, c] == 3).sum() / K - mean) <= 6.0 * np.sqrt(var / K)


@pytest.mark.parametrize("lds_width", [13, 14])
def test_toric_L5_samples_keep_syndrome_and_class(T, lds_width):
    m = errors(TORIC, 5, 1, 5)
    post, cls, z = twin(T, TORIC, 5, m, w=FLAT, K=64, mode=1, lds_width=lds_width)
    got = post[0].reshape(64, 2, 5, 5)
    assert np.array_equal(classes(TORIC, got), cls[0])
    assert np.array_equal(syndromes(TORIC, got), np.broadcast_to(syndromes(TORIC, m)[0], (64,) + syndromes(TORIC, m)[0].shape))
    assert len(np.unique(post[0], axis=0)) > 32                                 # independent draws, not one chain


# ------------------------------------------------------------------------------------------------------ the address
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 5, 0), (TORIC, 3, 6)])
def test_a_sample_is_a_function_of_its_address(T, code, L, lds_width):
    m = errors(code, L, 4, 3)
    kw = dict(w=DEPOL, lds_width=lds_width)
    full, _, _ = twin(T, code, L, m, K=6, first=10, **kw)
    assert np.array_equal(twin(T, code, L, m, K=3, first=10, **kw)[0], full[:, :, :3])                      # K
    assert np.array_equal(twin(T, code, L, m[2:3], K=6, first=12, **kw)[0], full[2:3])                      # N, first_syndrome moved along
    assert np.array_equal(twin(T, code, L, m[[3, 1]], K=6, first=13, **kw)[0][0], full[3])                  # the order of the rows ...
    assert np.array_equal(twin(T, code, L, m[[1, 3]], K=6, first=11, **kw)[0][0], full[1])
    post, cls, _ = twin(T, code, L, m, K=6, first=10, mode=1, **kw)
    for s in range(4):
        assert all(np.array_equal(post[s, k], full[s, cls[s, k], k]) for k in range(6))
    assert not np.array_equal(twin(T, code, L, m, K=6, first=10, seed=SEED + 1, **kw)[0], full)             # seed
    assert not np.array_equal(twin(T, code, L, m, K=6, first=11, **kw)[0], full)                            # s
    assert not np.array_equal(full[:, :, 0], full[:, :, 1])                                                 # k
    same = np.broadcast_to(m[0], m.shape)                                                                   # one syndrome four times: s alone differs
    four = twin(T, code, L, same, K=6, first=10, **kw)[0]
    assert not np.array_equal(four[0], four[1])


# ------------------------------------------------------------------------------------------------------ the low-p limit
@pytest.mark.parametrize("code,L", [(ROTATED, 7), (ROTATED, 9), (TORIC, 5)])
def test_low_p_samples_are_the_shortest_chains(T, code, L):
    m = MT.low_weight_errors(code, L, 2, np.random.default_rng(L))
    want, cost, count, _ = MT.twin(T, code, L, m, (0, 1, 1, 1))
    out, _, _ = twin(T, code, L, m, w=ex.depolarizing_w4(1e-12), K=2)
    cells = qubit_cells(generators(code, L))
    assert (count == 1).any()
    for s in range(2):
        for c in range(out.shape[1]):
            for k in range(2):
                assert np.count_nonzero(out[s, c, k][cells]) == cost[s, c]
                if count[s, c] == 1:
                    assert np.array_equal(out[s, c, k], want[s, c])


# ------------------------------------------------------------------------------------------------------ site tables
def test_constant_rows_are_the_uniform_entry_point(T):
    for code, L, lds_width in [(ROTATED, 5, 0), (PLANAR, 3, 0), (TORIC, 3, 6)]:
        m = errors(code, L, 2, 21)
        nq = int(np.prod(state_shape(code, L)))
        for mode in (0, 1):
            a = twin(T, code, L, m, w=BIASED, K=5, mode=mode, lds_width=lds_width)
            b = twin(T, code, L, m, wq=np.broadcast_to(BIASED, (nq, 4)), K=5, mode=mode, lds_width=lds_width)
            c = twin(T, code, L, m, wq=np.broadcast_to(BIASED, (2, nq, 4)), K=5, mode=mode, lds_width=lds_width)
            for x, y, v in zip(a, b, c):
                assert x.tobytes() == y.tobytes() == v.tobytes()


def test_a_table_row_per_syndrome_is_addressed_by_s(T):
    code, L = XZZX, 5
    m = errors(code, L, 3, 4)
    rng = np.random.default_rng(8)
    tabs = rng.uniform(0.05, 1.0, size=(3, L * L, 4))
    both = twin(T, code, L, m, wq=tabs, K=4)
    for s in range(3):
        one = twin(T, code, L, m[s:s + 1], wq=tabs[s], K=4, first=s)
        assert one[0].tobytes() == both[0][s:s + 1].tobytes() and one[2].tobytes() == both[2][s:s + 1].tobytes()


def test_pure_erasure_is_exact(T):
    code, L, K = ROTATED, 3, 1 << 14
    rng = np.random.default_rng(2)
    erased = np.zeros((L, L), bool)
    erased.ravel()[[0, 1, 3, 4, 5, 7]] = True
    err = np.zeros((1, L, L), np.uint8)
    err[0][erased] = rng.integers(0, 4, size=int(erased.sum()))               # an error on the erased set: its syndrome has chains there
    tab = ex.erasure_site_w4([1.0, 0.0, 0.0, 0.0], erased).reshape(L * L, 4)
    post, cls, z = twin(T, code, L, err, wq=tab, K=K, mode=1)
    assert (post[0][:, ~erased.ravel()] == 0).all()                             # no sample carries an error outside the erased set
    law = U.class_law(code, L, err[0], tab)
    zs = np.array([zc for _, _, zc in law])
    assert np.array_equal(z[0], zs) and (zs > 0).any()                          # (counts of chains: exact in float64)
    for c, (chains, prob, zc) in enumerate(law):
        if zc > 0:
            live = prob > 0
            assert np.allclose(prob[live], 1.0 / live.sum())                    # every chain on the erased set is as likely as another
            check_law(U.counts_of(post[0][cls[0] == c], chains), prob, "erasure class %d" % c)
        else:
            assert not (cls[0] == c).any()                                      # a class of weight 0 is never drawn
    # every qubit erased: all chains of the syndrome are equally likely, and the four Paulis at a qubit are uniform
    full = twin(T, code, L, err, wq=np.ones((L * L, 4)), K=K, mode=1)[0][0]
    for q in range(L * L):
        check_law(np.bincount(full[:, q], minlength=4), np.full(4, 0.25), "full erasure, qubit %d" % q)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(T):
    m = errors(ROTATED, 3, 2, 1)
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, w=DEPOL, K=0)
    assert rc == -1 and msg.startswith("qecmc_class_sample: K=0")
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, w=DEPOL, K=1 << 32)
    assert rc == -1 and msg.startswith("qecmc_class_sample: K=4294967296")
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, w=DEPOL, K=1, mode=2)
    assert rc == -1 and "mode=2" in msg
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, w=DEPOL, K=1, first=(1 << 32) - 1)
    assert rc == -1 and "exceed 32 bits" in msg
    for bad, frag in ((np.inf, "w[1]=inf"), (-0.5, "w[1]=-0.5"), (np.nan, "w[1]=nan")):
        rc, msg, *_ = twin_rc(T, ROTATED, 3, m, w=[1.0, bad, 0.1, 0.1], K=1)
        assert rc == -1 and msg.startswith("qecmc_class_sample: ") and frag in msg
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, w=[0.0, 0.0, 0.0, 0.0], K=1)
    assert rc == -1 and "all zero" in msg
    # a zero class in mode 0 names the row and the class; mode 1 draws from the classes that are left
    zero = np.zeros((2, 3, 3), np.uint8)
    zero[1, 0, 0] = 1
    only_identity = [1.0, 0.0, 0.0, 0.0]
    rc, msg, _, _, z = twin_rc(T, ROTATED, 3, zero, w=only_identity, K=1)
    assert rc == -1 and msg.startswith("qecmc_class_sample: row 0, class 1:") and z[0, 0] == 1.0
    rc, msg, out, cls, z = twin_rc(T, ROTATED, 3, zero[:1], w=only_identity, K=3, mode=1)
    assert rc == 0 and (cls == 0).all() and (out == 0).all()
    rc, msg, *_ = twin_rc(T, ROTATED, 3, zero, w=only_identity, K=3, mode=1)    # row 1 has an X: no chain of any class is the identity everywhere
    assert rc == -1 and msg.startswith("qecmc_class_sample: row 1: the class weights total 0")
    rc, msg, *_ = twin_rc(T, ROTATED, 3, zero, w=[1e300, 1e300, 1e300, 1e300], K=1, mode=1)
    assert rc == -1 and "row 0" in msg and "inf" in msg
    # the site form, under its own name
    tab = np.ones((9, 4))
    tab[4] = 0.0
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, wq=tab, K=1)
    assert rc == -1 and msg.startswith("qecmc_class_sample_site: ") and "qubit 4" in msg
    rc, msg, *_ = twin_rc(T, ROTATED, 3, errors(ROTATED, 3, 3, 1), wq=np.ones((2, 9, 4)), K=1)
    assert rc == -1 and msg.startswith("qecmc_class_sample_site: wq_rows=2")


@pytest.mark.parametrize("code,L,lds_width", [(TORIC, 4, 0), (TORIC, 7, 0), (ROTATED, 13, 0), (PLANAR, 8, 0), (ROTATED, 5, 1), (ROTATED, 5, 15), (ROTATED, 4, 0), (7, 3, 0),
                                              (TORIC, 5, 3)])
def test_every_cut_plan_refusal_under_the_new_name(T, code, L, lds_width):
    rc_cut, _, cut_msg = SC.info(T, code, L, lds_width)
    assert rc_cut != 0
    nq = int(np.prod(state_shape(code, L))) if code in (TORIC, XZZX, ROTATED, PLANAR) else 9
    m = np.zeros((1, nq), np.uint8)
    for kw, name in ((dict(w=DEPOL), "qecmc_class_sample"), (dict(wq=np.ones((nq, 4))), "qecmc_class_sample_site")):
        out = np.zeros((1, 16, 1, nq), np.uint8)
        cls, z, msg = np.zeros((1, 1), np.int32), np.zeros((1, 16)), C.create_string_buffer(640)
        w = None if "w" not in kw else np.ascontiguousarray(kw["w"])
        tab = None if "wq" not in kw else np.ascontiguousarray(kw["wq"])
        rc = T.qt_class_sample(code, L, 1, m.ctypes.data_as(_u8p), None if w is None else w.ctypes.data_as(_f64p), None if tab is None else tab.ctypes.data_as(_f64p),
                               0 if tab is None else 1, lds_width, 1, 0, 0, 0, out.ctypes.data_as(_u8p), cls.ctypes.data_as(_i32p), z.ctypes.data_as(_f64p), msg, 640)
        assert rc == rc_cut and msg.value.decode() == name + ": " + cut_msg.decode()


def test_python_layer_refuses_before_a_device_is_looked_for():
    with pytest.raises(L_.QecmcError, match="qecmc_class_sample: .*no class move"):
        ex.sample_chains("toric", np.zeros((1, 2, 4, 4), np.uint8), p=0.1)
    with pytest.raises(L_.QecmcError, match="qecmc_class_sample_site: lds_width=1"):
        ex.sample_chains_site("rotated", np.zeros((1, 3, 3), np.uint8), np.ones((3, 3, 4)), lds_width=1)
    with pytest.raises(L_.QecmcError, match="qecmc_class_sample: w\\[2\\]=-1"):
        ex.sample_posterior("rotated", np.zeros((1, 3, 3), np.uint8), w4=[1, 1, -1, 1])
    with pytest.raises(ValueError, match="n_samples"):
        ex.sample_chains("rotated", np.zeros((1, 3, 3), np.uint8), p=0.1, n_samples=0)
    with pytest.raises(ValueError, match="either p"):
        ex.sample_chains("rotated", np.zeros((1, 3, 3), np.uint8))
    with pytest.raises(ValueError, match="replace"):
        ex.sample_posterior("rotated", np.zeros((1, 3, 3), np.uint8), p=0.1, site_weights=np.ones((3, 3, 4)))
