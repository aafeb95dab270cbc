"""The exact per-qubit marginals (csrc/class_marginal.hpp), without a GPU: the twin, compiled by g++ into the host-table test library
(qt_class_marginals, qt_class_marginals_plan, qt_class_marginals_group), and the Python layer around it.

What is pinned: THE CONDITIONING IDENTITY -- weights[s, c, q, P] is the class weight of the site twin under a table whose row q keeps w[P] at P and 0
elsewhere: an independent yardstick, which knows no backward sweep and no fold --; the brute force of tests/util_class_sample.py summed per qubit and
Pauli; the four weights of a qubit total z; z is the cut twin's, bit for bit; held generators; the class and the syndrome alone decide; the lower
bound the shortest chain sets; pure erasure, exactly; the sampler's twin, by counts; every refusal by name; exact_error_counts.  (The sanitizers and
the resource tables: tests/test_class_marginal_resources.py.)

THE TOLERANCE is derived, not measured.  Every compared quantity is a sum of products of non-negative doubles, so its relative error is at most
d u (1 + O(d u)), u = 2^-53, d the number of roundings along a path: n_ops multiplies and adds forward, n_ops backward, the product d[f], 2^width / 64
adds of a fold lane and 6 of the butterfly, n_held adds over the held generators; the scale is a power of two.  d = 2 n_ops + 2^width / 64 + n_held + 16
bounds that, and two quantities are compared with rtol = 2 d u.  An exact 0 on one side must be an exact 0 on the other."""
import ctypes as C
import statistics

import numpy as np
import pytest

import test_class_minplus_trace_cpu as MT
import test_class_sample_cpu as SA
import test_class_sweep_cut_cpu as SC
import test_class_sweep_site_cpu as SS
import util_class_sample as U
from qecmc import _lib as L_
from qecmc import exact as ex
from test_corrections_cpu import apply_kind, classes, generators
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_minplus_trace import qubit_cells

NAME = MT.NAME
WORKSPACE = 512 << 20
FOLD_BYTES = 64 << 20
_u8p, _u32p, _i32p, _u64p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
DEPOL = ex.depolarizing_w4(0.1)
BIASED = ex.biased_w4(0.1, 10.0)
WITH_ZERO = np.array([1.0, 0.3, 0.0, 0.2])
U53 = 2.0 ** -53


def load_twin():
    """the host-table test library with the marginals' entry points (tests/test_gpu_class_marginal.py compares the GPU with it)"""
    lib = SA.load_twin()
    lib.qt_class_marginals.restype = C.c_int
    lib.qt_class_marginals.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _f64p, _f64p, C.c_uint64, C.c_int, _f64p, _f64p, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_marginals_plan.restype = C.c_int
    lib.qt_class_marginals_plan.argtypes = [C.c_int, C.c_int, C.c_int, _u32p, C.c_int, _u64p]
    lib.qt_class_marginals_group.restype = None
    lib.qt_class_marginals_group.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint64, _u32p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def nq_of(code, L):
    return int(np.prod(state_shape(code, L)))


def twin_rc(T, code, L, chains, w=None, wq=None, lds_width=0, n=None):
    """(rc, message, weights float64[N, ncls, nq, 4], z float64[N, ncls], cls int32[N]) of the host twin; the outputs start out poisoned.
    wq: float[rows, nq, 4] or [nq, 4]"""
    nq = nq_of(code, L) if 2 <= L <= 64 and code in (TORIC, XZZX, ROTATED, PLANAR) else 1
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    n, ncls = len(flat) if n is None else n, 16 if code == TORIC else 4
    rows = min(n, len(flat))
    out, z, cls = np.full((rows, ncls, nq, 4), -7.0), np.full((rows, ncls), -1.0), np.full(rows, 9, np.int32)
    msg = C.create_string_buffer(640)
    wp = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    tab = None if wq is None else np.ascontiguousarray(wq, dtype=np.float64).reshape(-1, nq, 4)
    rc = T.qt_class_marginals(code, L, n, flat.ctypes.data_as(_u8p), None if wp is None else wp.ctypes.data_as(_f64p), None if tab is None else tab.ctypes.data_as(_f64p),
                              0 if tab is None else len(tab), lds_width, out.ctypes.data_as(_f64p), z.ctypes.data_as(_f64p), cls.ctypes.data_as(_i32p), msg, 640)
    return rc, msg.value.decode(), out, z, cls


def twin(T, code, L, chains, **kw):
    rc, msg, out, z, cls = twin_rc(T, code, L, chains, **kw)
    assert rc == 0, msg
    return out, z, cls


def plan_numbers(T, code, L, lds_width):
    out8 = np.zeros(8, np.uint64)
    close = np.zeros(512, np.uint32)
    n = T.qt_class_marginals_plan(code, L, lds_width, close.ctypes.data_as(_u32p), close.size, out8.ctypes.data_as(_u64p))
    assert n >= 0
    d = dict(zip(("width", "held", "n_close", "job_bytes", "workspace", "fold_bytes", "n_ops", "nq"), (int(x) for x in out8)))
    d["close_qubit"] = close[:n].copy()
    return d


def group_of(T, n, ncls, pn):
    g = np.zeros(2, np.uint32)
    T.qt_class_marginals_group(n, ncls, pn["held"], pn["n_close"], pn["job_bytes"], g.ctypes.data_as(_u32p))
    return int(g[0]), int(g[1])


def rtol_of(T, code, L, lds_width=0):
    pn = plan_numbers(T, code, L, lds_width)
    d = 2 * pn["n_ops"] + (1 << pn["width"]) // 64 + pn["held"] + 16
    return 2.0 * d * U53


def close_to(a, b, rtol):
    """every pair within rtol of the larger, and a zero on one side a zero on the other"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a == 0.0, b == 0.0) and bool((np.abs(a - b) <= rtol * np.maximum(a, b)).all())


def errors(code, L, n, seed):
    return random_errors(code, L, n, np.random.default_rng([91, seed]))


# ------------------------------------------------------------------------------------------------------ the plan's numbers
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 3, 0), (ROTATED, 9, 0), (ROTATED, 11, 0), (PLANAR, 4, 0), (PLANAR, 7, 0), (TORIC, 3, 6), (TORIC, 5, 13), (TORIC, 5, 14)])
def test_record_bytes_and_launch_group(T, code, L, lds_width):
    _, inf, _ = SC.info(T, code, L, lds_width)
    pn = plan_numbers(T, code, L, lds_width)
    cells = np.flatnonzero(qubit_cells(generators(code, L)))
    print(NAME[code], L, lds_width, {k: v for k, v in pn.items() if k != "close_qubit"})
    assert pn["width"] == inf["width"] and pn["held"] == inf["held"] and pn["n_ops"] == inf["n_ops"] and pn["workspace"] == WORKSPACE and pn["fold_bytes"] == FOLD_BYTES
    assert sorted(pn["close_qubit"].tolist()) == cells.tolist()                # every cell that holds a qubit is closed once
    assert pn["job_bytes"] == pn["n_close"] * (1 << inf["width"]) * 8
    per_syndrome = inf["ncls"] << inf["held"]
    for n in (1, 2, 40, 5000, 1 << 32):
        S, jobs = group_of(T, n, inf["ncls"], pn)
        assert 1 <= S <= T.qt_class_sweep_cut_group(n, inf["ncls"], inf["held"]) and S <= max(n, 1)
        assert 1 <= jobs <= min(S * per_syndrome, 1 << 16) and jobs * pn["job_bytes"] <= WORKSPACE
        assert S == 1 or S * per_syndrome * pn["n_close"] * 32 <= FOLD_BYTES
    big = group_of(T, 1 << 32, inf["ncls"], pn)
    assert group_of(T, 1 << 20, inf["ncls"], pn) == big                         # nothing grows with N


# ------------------------------------------------------------------------------------------------------ 1. the conditioning identity
def conditioned_z(T, code, L, chain, w, q, P, lds_width=0):
    """Z of every class under the table whose row q keeps w[P] at P and 0 elsewhere: the site twin of the cut route"""
    tab = np.broadcast_to(np.asarray(w, dtype=np.float64), (nq_of(code, L), 4)).copy()
    keep = tab[q, P]
    tab[q] = 0.0
    tab[q, P] = keep
    return SS.twin(T, "cut", code, L, chain, tab, (lds_width,))[0][0]


@pytest.mark.parametrize("code,L,w", [(TORIC, 3, DEPOL), (PLANAR, 3, BIASED), (XZZX, 3, WITH_ZERO), (ROTATED, 3, BIASED), (ROTATED, 5, DEPOL), (XZZX, 5, BIASED)])
def test_conditioning_identity_at_every_qubit_and_pauli(T, code, L, w):
    m = errors(code, L, 1, L + code)
    out, z, _ = twin(T, code, L, m, w=w)
    rtol = rtol_of(T, code, L)
    for q in np.flatnonzero(qubit_cells(generators(code, L))):
        for P in range(4):
            if w[P] == 0.0:
                assert (out[0, :, q, P] == 0.0).all()                           # (a row of four zeros is refused by the site twin: the marginal is an exact 0)
                continue
            assert close_to(out[0, :, q, P], conditioned_z(T, code, L, m, w, q, P), rtol), (q, P)


@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 7, 0), (TORIC, 5, 13), (TORIC, 5, 14)])
def test_conditioning_identity_at_32_random_cells(T, code, L, lds_width):
    m = errors(code, L, 1, 40 + L)
    out, z, _ = twin(T, code, L, m, w=DEPOL, lds_width=lds_width)
    rtol = rtol_of(T, code, L, lds_width)
    rng = np.random.default_rng([92, code, L, lds_width])
    cells = np.flatnonzero(qubit_cells(generators(code, L)))
    for _ in range(32):
        q, P = int(rng.choice(cells)), int(rng.integers(0, 4))
        assert close_to(out[0, :, q, P], conditioned_z(T, code, L, m, DEPOL, q, P, lds_width), rtol), (q, P)
    assert close_to(out[0].sum(axis=2)[:, cells], np.broadcast_to(z[0][:, None], (z.shape[1], len(cells))), rtol + 4 * U53)


# ------------------------------------------------------------------------------------------------------ 2, 3, 10. the brute force; the totals; z
def brute_marginals(code, L, chain, w):
    """float64[ncls, nq, 4] and Z float64[ncls] from the enumerated law: chains and probabilities summed per qubit and Pauli"""
    with np.errstate(invalid="ignore"):                                         # (the law of a class of weight 0 is 0 / 0: only its chains and its Z are used)
        law = U.class_law(code, L, chain, w)
    nq, gens = nq_of(code, L), generators(code, L)
    out = np.zeros((len(law), nq, 4))
    for c, (chains, prob, zc) in enumerate(law):
        wt = U.chain_weights(gens, chains, w).astype(np.longdouble)            # the reference's own error: nq roundings of the product, and sums of up to
        for P in range(4):                                                      # 2^16 terms in extended precision along the contiguous axis (pairwise): far below d u
            out[c, :, P] = np.ascontiguousarray(((chains == P) * wt[:, None]).T).sum(axis=1)
    return out, np.array([zc for _, _, zc in law])


@pytest.mark.parametrize("code", [TORIC, XZZX, ROTATED, PLANAR])
def test_brute_force_at_L3(T, code):
    w = BIASED if code != PLANAR else DEPOL
    m = errors(code, 3, 2, 7 + code)
    out, z, cls = twin(T, code, 3, m, w=w)
    rtol = rtol_of(T, code, 3)
    assert z.tobytes() == SC.twin(T, code, 3, m, w)[0].tobytes() and np.array_equal(cls, classes(code, m))
    cells = qubit_cells(generators(code, 3))
    for s in range(2):
        want, zs = brute_marginals(code, 3, m[s], w)
        assert close_to(z[s], zs, rtol)
        assert close_to(out[s][:, cells], want[:, cells], rtol)
        assert close_to(out[s][:, cells].sum(axis=2), np.broadcast_to(z[s][:, None], (len(zs), int(cells.sum()))), rtol + 4 * U53)
        for q in np.flatnonzero(~cells):                                        # a cell that holds no qubit: z at the input's byte there, 0 elsewhere
            for c in range(len(zs)):
                assert out[s, c, q, m[s].ravel()[q]] == z[s, c] and np.count_nonzero(out[s, c, q]) == (z[s, c] != 0)


@pytest.mark.parametrize("code,L", [(ROTATED, 5), (PLANAR, 4), (ROTATED, 7)])
def test_the_four_weights_total_z_and_z_is_the_cut_twins(T, code, L):
    m = errors(code, L, 2, 3)
    for w in (DEPOL, WITH_ZERO):
        out, z, _ = twin(T, code, L, m, w=w)
        assert z.tobytes() == SC.twin(T, code, L, m, w)[0].tobytes() if (w > 0).all() else True
        cells = qubit_cells(generators(code, L))
        tot = out[:, :, cells].sum(axis=3)
        assert close_to(tot, np.broadcast_to(z[:, :, None], tot.shape), rtol_of(T, code, L) + 4 * U53)
        assert (out >= 0.0).all()


@pytest.mark.parametrize("code", [TORIC, ROTATED, PLANAR])
def test_exact_error_counts_against_the_brute_force(T, code, monkeypatch):
    n = 1 if code == TORIC else 2                                               # (the enumeration of the 16 toric classes is the slow part)
    m = errors(code, 3, n, 17)
    p = 0.13

    def through_the_twin(code_, chains, w, site_weights, size, lds_width):     # the Python layer on the twin's numbers: no device here
        out, z, cls = twin(T, code_, 3, chains, w=w, lds_width=lds_width)
        return dict(weights=out.reshape(out.shape[:2] + state_shape(code_, 3) + (4,)), z=z, cls=cls, width=0, held=0)
    monkeypatch.setattr(ex, "_marginals", through_the_twin)
    got = ex.exact_error_counts(code, m, p)
    assert got["per_class"].shape == (n, 16 if code == TORIC else 4) and got["posterior"].shape == (n,)
    for s in range(n):
        law = U.class_law(code, 3, m[s], ex.depolarizing_w4(p))
        cells = qubit_cells(generators(code, 3))
        per = np.array([(prob * np.count_nonzero(chains[:, cells], axis=1)).sum() for chains, prob, _ in law])
        zs = np.array([zc for _, _, zc in law])
        assert np.allclose(got["per_class"][s], per, rtol=1e-12, atol=1e-13)
        assert abs(got["posterior"][s] - (per * zs).sum() / zs.sum()) <= 1e-12


# ------------------------------------------------------------------------------------------------------ 4. held generators
@pytest.mark.parametrize("lds_width", [6, 9])
def test_held_generators_at_toric_L3_against_the_default_route(T, lds_width):
    m = errors(TORIC, 3, 2, 5)
    assert plan_numbers(T, TORIC, 3, lds_width)["held"] > 0 and plan_numbers(T, TORIC, 3, 0)["held"] == 0
    a, za, _ = twin(T, TORIC, 3, m, w=BIASED, lds_width=lds_width)
    b, zb, _ = twin(T, TORIC, 3, m, w=BIASED)
    rtol = max(rtol_of(T, TORIC, 3, lds_width), rtol_of(T, TORIC, 3, 0))
    assert close_to(a, b, rtol) and close_to(za, zb, rtol)
    assert za.tobytes() == SC.twin(T, TORIC, 3, m, BIASED, lds_width)[0].tobytes()


def test_held_generators_at_toric_L5_widths_13_and_14(T):
    m = errors(TORIC, 5, 1, 6)
    a, za, _ = twin(T, TORIC, 5, m, w=DEPOL, lds_width=13)
    b, zb, _ = twin(T, TORIC, 5, m, w=DEPOL, lds_width=14)
    assert plan_numbers(T, TORIC, 5, 13)["held"] == 8 and plan_numbers(T, TORIC, 5, 14)["held"] == 7
    rtol = max(rtol_of(T, TORIC, 5, 13), rtol_of(T, TORIC, 5, 14))
    assert close_to(a, b, rtol) and close_to(za, zb, rtol)


# ------------------------------------------------------------------------------------------------------ 5. the class and the syndrome alone
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 5, 0), (PLANAR, 4, 0), (TORIC, 3, 6)])
def test_the_class_and_the_syndrome_alone_decide(T, code, L, lds_width):
    rng = np.random.default_rng([93, code])
    m = errors(code, L, 1, 9)
    gens = generators(code, L)
    moved = m.reshape(1, -1).copy()
    for g in gens[rng.random(len(gens)) < 0.5]:
        moved ^= g
    rtol = rtol_of(T, code, L, lds_width)
    a, za, ca = twin(T, code, L, m, w=BIASED, lds_width=lds_width)
    b, zb, cb = twin(T, code, L, moved, w=BIASED, lds_width=lds_width)
    cells = qubit_cells(gens)
    assert close_to(a[:, :, cells], b[:, :, cells], rtol) and close_to(za, zb, rtol) and ca[0] == cb[0]
    for kind in range(4 if code == TORIC else 2):                               # a logical operator: the same sets of chains, the input in another class
        other = np.asarray(apply_kind(code, m[0], kind), dtype=np.uint8)[None]
        c, zc, cc = twin(T, code, L, other, w=BIASED, lds_width=lds_width)
        assert cc[0] == classes(code, other)[0] != ca[0]
        assert close_to(a[:, :, cells], c[:, :, cells], rtol) and close_to(za, zc, rtol)     # weights[s, c] belongs to class c, as eq_class numbers it, whatever the input's


# ------------------------------------------------------------------------------------------------------ 6. the shortest chain's lower bound
@pytest.mark.parametrize("code,L", [(ROTATED, 7), (TORIC, 5)])
def test_lower_bound_from_the_shortest_chain(T, code, L):
    m = MT.low_weight_errors(code, L, 1, np.random.default_rng(L))
    short, cost, count, _ = MT.twin(T, code, L, m, (0, 1, 1, 1))
    cells = np.flatnonzero(qubit_cells(generators(code, L)))
    rtol = rtol_of(T, code, L)
    w = DEPOL
    out, z, _ = twin(T, code, L, m, w=w)
    for c in range(z.shape[1]):
        floor = float(np.prod(w[short[0, c][cells]])) / z[0, c]               # the chain alone is this much of its class
        mine = out[0, c, cells, short[0, c][cells]] / z[0, c]
        assert (mine >= floor * (1.0 - 4.0 * rtol)).all() and (mine <= 1.0 + 4.0 * rtol).all()
    low, zl, _ = twin(T, code, L, m, w=ex.depolarizing_w4(1e-12))
    assert (count[0] == 1).any()
    for c in range(z.shape[1]):
        if count[0, c] == 1:
            assert np.array_equal(low[0, c, cells].argmax(axis=1), short[0, c][cells])


# ------------------------------------------------------------------------------------------------------ 7. pure erasure
def test_pure_erasure_is_exact(T, monkeypatch):
    code, L = ROTATED, 3
    rng = np.random.default_rng(2)
    erased = np.zeros((L, L), bool)
    erased.ravel()[[0, 1, 2, 3, 4]] = True                                      # a whole row, so that one logical operator fits the erased set and the other does not
    err = np.zeros((1, L, L), np.uint8)
    err[0][erased] = rng.integers(0, 4, size=int(erased.sum()))
    tab = ex.erasure_site_w4([1.0, 0.0, 0.0, 0.0], erased).reshape(L * L, 4)
    out, z, _ = twin(T, code, L, err, wq=tab)
    with np.errstate(invalid="ignore"):                                         # (the law of a class of weight 0 is 0 / 0: only its Z is used)
        law = U.class_law(code, L, err[0], tab)
    zs = np.array([zc for _, _, zc in law])
    assert np.array_equal(z[0], zs) and (zs > 0).any() and (zs == 0).any()      # (counts of chains: exact in float64)
    off = ~erased.ravel()
    assert out[0][:, off, 0].tobytes() == np.repeat(z[0][:, None], int(off.sum()), axis=1).tobytes()      # off the erased set: I with weight z, as bits
    assert (out[0][:, off, 1:] == 0.0).all()
    assert (out[0][zs == 0] == 0.0).all()                                       # a class of weight 0: all zeros
    want, _ = brute_marginals(code, L, err[0], tab)
    assert np.array_equal(out[0], want)                                         # counts of chains: exact
    def through_the_twin(code_, chains, w, site_weights, size, lds_width):
        return dict(weights=out.reshape((1, 4, L, L, 4)), z=z, cls=np.zeros(1, np.int32), width=0, held=0)
    monkeypatch.setattr(ex, "_marginals", through_the_twin)
    dead = int(np.flatnonzero(zs == 0)[0])
    with pytest.raises(FloatingPointError, match="row 0, class %d" % dead):
        ex.class_marginals_site("rotated", err, tab.reshape(L, L, 4))
    assert ex.class_marginals_site("rotated", err, tab.reshape(L, L, 4), normalize=False)["weights"].shape == (1, 4, L, L, 4)
    post = ex.posterior_marginals("rotated", err, site_weights=tab.reshape(L, L, 4))
    assert post.shape == (1, L, L, 4) and np.allclose(post.sum(axis=-1), 1.0) and (post[0][~erased][:, 0] == 1.0).all()


# ------------------------------------------------------------------------------------------------------ 8. the sampler's twin
def test_counts_of_the_samplers_twin_against_the_marginals(T):
    """K = 2^14 draws per class at rotated L = 5: per cell (s, c, q, P) that expects at least 5 draws, z = (count - K m) / sqrt(K m (1 - m)); the largest
    |z| stays within the two-sided 1 - 1e-6 normal quantile, Bonferroni over the cells.  Deterministic under SA.SEED"""
    code, L, K = ROTATED, 5, 1 << 14
    m = errors(code, L, 2, 12)
    out, z, _ = twin(T, code, L, m, w=DEPOL)
    draws, _, zs = SA.twin(T, code, L, m, w=DEPOL, K=K)
    assert zs.tobytes() == z.tobytes()
    marg = out / z[:, :, None, None]
    counts = np.stack([(draws == P).sum(axis=2) for P in range(4)], axis=-1)    # [N, ncls, nq, 4]
    use = K * marg >= 5.0
    zscore = (counts[use] - K * marg[use]) / np.sqrt(K * marg[use] * np.maximum(1.0 - marg[use], U53))
    sure = marg[use] >= 1.0 - 1e-15
    bound = statistics.NormalDist().inv_cdf(1.0 - 0.5e-6 / int(use.sum()))
    print("cells %d, largest |z| %.2f, bound %.2f" % (int(use.sum()), np.abs(zscore[~sure]).max(), bound))
    assert np.abs(zscore[~sure]).max() <= bound and (counts[use][sure] == K).all()
    assert (counts[~use & (marg == 0.0)] == 0).all()


def dense_errors(code, L, n):
    """n errors at rate 0.2 per qubit, none of them empty.  The bound below takes its error bar from the draws, so it needs syndromes whose posterior is
    not all but a point mass: under a trivial syndrome at p = 0.1 1 024 draws can all be the empty chain, and their std is 0"""
    rng = np.random.default_rng([94, code, L, 6])
    cells = qubit_cells(generators(code, L))
    m = np.zeros((n, len(cells)), np.uint8)
    for row in m:
        while not row.any():
            hit = cells & (rng.random(len(cells)) < 0.2)
            row[hit] = rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)
    return m.reshape((n,) + state_shape(code, L))


@pytest.mark.parametrize("code,L", [(TORIC, 3), (ROTATED, 7)])
def test_exact_count_against_the_samplers_twin(T, code, L):
    """what tests/test_gpu_class_marginal.py::test_exact_error_count_against_exact_draws asks of the GPU, on the twins and on the same chains: per
    syndrome |exact - mean of 1 024 draws| <= 5 std / sqrt(1024), the std taken from the draws"""
    m, p, K = dense_errors(code, L, 8), 0.1, 1024
    w = ex.depolarizing_w4(p)
    out, z, _ = twin(T, code, L, m, w=w)
    exact = (1.0 - out.sum(axis=1)[:, :, 0] / z.sum(axis=1)[:, None]).sum(axis=1)
    draws = SA.twin(T, code, L, m, w=w, K=K, mode=1)[0]
    n_err = (draws != 0).sum(axis=2)
    bar = n_err.std(axis=1, ddof=1) / np.sqrt(K)
    print("exact", exact, "draws", n_err.mean(axis=1), "|d| / bar", np.abs(exact - n_err.mean(axis=1)) / bar)
    assert (bar > 0).all() and (np.abs(exact - n_err.mean(axis=1)) <= 5.0 * bar).all()


# ------------------------------------------------------------------------------------------------------ 9. refusals; the Python layer
def test_refusals_by_name(T):
    m = errors(ROTATED, 3, 2, 1)
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m[:1], w=DEPOL, n=1 << 32)
    assert rc == -1 and msg.startswith("qecmc_class_marginals: N=4294967296")
    for bad, frag in ((np.inf, "w[1]=inf"), (-0.5, "w[1]=-0.5"), (np.nan, "w[1]=nan")):
        rc, msg, *_ = twin_rc(T, ROTATED, 3, m, w=[1.0, bad, 0.1, 0.1])
        assert rc == -1 and msg.startswith("qecmc_class_marginals: ") and frag in msg
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, w=[0.0, 0.0, 0.0, 0.0])
    assert rc == -1 and "all zero" in msg
    rc, msg, out, z, _ = twin_rc(T, ROTATED, 3, np.zeros((1, 3, 3), np.uint8), w=[1.0, 0.0, 0.0, 0.0])       # single zeros are allowed: a class of weight 0 comes back as zeros
    assert rc == 0 and z[0].tolist() == [1.0, 0.0, 0.0, 0.0] and (out[0, 1:] == 0.0).all() and (out[0, 0, :, 0] == 1.0).all()
    tab = np.ones((9, 4))
    tab[4] = 0.0
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, wq=tab)
    assert rc == -1 and msg.startswith("qecmc_class_marginals_site: ") and "qubit 4" in msg
    rc, msg, *_ = twin_rc(T, ROTATED, 3, errors(ROTATED, 3, 3, 1), wq=np.ones((2, 9, 4)))
    assert rc == -1 and msg.startswith("qecmc_class_marginals_site: wq_rows=2")
    tab = np.ones((9, 4))
    tab[2, 1] = -1.0
    rc, msg, *_ = twin_rc(T, ROTATED, 3, m, wq=tab)
    assert rc == -1 and msg.startswith("qecmc_class_marginals_site: ") and "qubit 2" in msg


@pytest.mark.parametrize("code,L,lds_width", [(TORIC, 4, 0), (TORIC, 7, 0), (ROTATED, 13, 0), (PLANAR, 8, 0), (ROTATED, 5, 1), (ROTATED, 5, 15), (ROTATED, 4, 0), (7, 3, 0),
                                              (TORIC, 5, 3)])
def test_every_cut_plan_refusal_under_the_new_names(T, code, L, lds_width):
    rc_cut, _, cut_msg = SC.info(T, code, L, lds_width)
    assert rc_cut != 0
    nq = nq_of(code, L) if code in (TORIC, XZZX, ROTATED, PLANAR) else 9
    m = np.zeros((1, nq), np.uint8)
    f64p = C.POINTER(C.c_double)
    for site, name in ((False, "qecmc_class_marginals"), (True, "qecmc_class_marginals_site")):
        out, z, msg = np.zeros((1, 16, nq, 4)), np.zeros((1, 16)), C.create_string_buffer(640)
        w, tab = np.ascontiguousarray(DEPOL), np.ones((nq, 4))
        rc = T.qt_class_marginals(code, L, 1, m.ctypes.data_as(_u8p), None if site else w.ctypes.data_as(_f64p), tab.ctypes.data_as(_f64p) if site else None, 1 if site else 0,
                                  lds_width, out.ctypes.data_as(_f64p), z.ctypes.data_as(_f64p), None, msg, 640)
        assert rc == rc_cut and msg.value.decode() == name + ": " + cut_msg.decode()
        # ... and the library, without a device: the same code and the same words
        lib = L_.lib()
        if site:
            got = lib.qecmc_class_marginals_site(code, L, 1, L_.u8(m), tab.ctypes.data_as(f64p), 1, lds_width, out.ctypes.data_as(f64p), z.ctypes.data_as(f64p), None)
        else:
            got = lib.qecmc_class_marginals(code, L, 1, L_.u8(m), w.ctypes.data_as(f64p), lds_width, out.ctypes.data_as(f64p), z.ctypes.data_as(f64p), None)
        assert got == rc_cut and lib.qecmc_last_error().decode() == name + ": " + cut_msg.decode()


def test_python_layer_refuses_before_a_device_is_looked_for():
    zero = np.zeros((1, 3, 3), np.uint8)
    with pytest.raises(L_.QecmcError, match="qecmc_class_marginals: .*no class move"):
        ex.class_marginals("toric", np.zeros((1, 2, 4, 4), np.uint8), p=0.1)
    with pytest.raises(L_.QecmcError, match="qecmc_class_marginals_site: lds_width=1"):
        ex.class_marginals_site("rotated", zero, np.ones((3, 3, 4)), lds_width=1)
    with pytest.raises(L_.QecmcError, match="qecmc_class_marginals: w\\[2\\]=-1"):
        ex.posterior_marginals("rotated", zero, w4=[1, 1, -1, 1])
    with pytest.raises(L_.QecmcError, match="qecmc_class_marginals: .*all zero"):
        ex.class_marginals("rotated", zero, w4=[0, 0, 0, 0])
    with pytest.raises(L_.QecmcError, match="qecmc_class_marginals_site: wq\\[row 0\\]\\[qubit 4\\]"):
        ex.class_marginals_site("rotated", zero, np.where(np.arange(9).reshape(3, 3, 1) == 4, 0.0, np.ones((3, 3, 4))))
    with pytest.raises(ValueError, match="either p"):
        ex.class_marginals("rotated", zero)
    with pytest.raises(ValueError, match="replace"):
        ex.posterior_marginals("rotated", zero, p=0.1, site_weights=np.ones((3, 3, 4)))
    with pytest.raises(ValueError, match="site_weights of shape"):
        ex.class_marginals_site("rotated", zero, np.ones((2, 3, 3, 4)))
    with pytest.raises(ValueError, match="not \\[N, ...\\] configurations"):
        ex.class_marginals("rotated", np.zeros((1, 3, 4), np.uint8), p=0.1)
    import qecmc
    for name in ("class_marginals", "class_marginals_site", "posterior_marginals", "exact_error_counts"):
        assert getattr(qecmc, name) is getattr(ex, name) and name in qecmc.__all__
    assert "exact_error_counts" in ex.posterior_error_counts.__doc__ and "posterior_error_counts" in ex.exact_error_counts.__doc__
