"""The service kernels at the top of the accepted range: shapes, the branch each one takes, and the batches that
tests/test_large_lattice_cpu.py (the g++ twins against the oracle) and tests/test_gpu_large_lattice.py (the GPU against the twins and the oracle)
share.  Everything here reads the oracle and the host twins only.

k_syndrome_lift and k_corrections keep W * 64 state words in dynamic LDS, W = ceil(nq / 16): up to 65 536 bytes a launch runs in the default
window, beyond it only after the launcher has raised the kernel's limit.  BRANCH is the table of the shapes on either side of that line and at
the top; on_branch() checks a shape against it from the twin's own table, so that a change of layout cannot quietly move a shape elsewhere.

The helpers of test_syndrome_lift_cpu.py / test_corrections_cpu.py form dense [N, n_gen, nq] arrays; here a generator is its four sites
(generator_sites), and the energy change of every generator on every chain is taken from those (generator_changes)."""
import functools

import numpy as np

import test_corrections_cpu as corr_cpu
import test_syndrome_lift_cpu as lift_cpu
from oracle import oracle as orc
from test_syndrome_lift_cpu import ORC_CODE, PLANAR, ROTATED, TORIC, XZZX, _u32p, n_cells, oracle_syndrome, state_shape

N = 70                                                                # two wavefronts, the second ragged
DEFAULT_WINDOW = 64 * 1024                                            # dynamic LDS a kernel may ask for without an opt-in
# (code, L) -> (W, LDS bytes): the last shapes inside the default window, the first through the opt-in, the top of the range
BRANCH = {(TORIC, 45): (254, 65024), (XZZX, 63): (249, 63744), (ROTATED, 63): (249, 63744),
          (TORIC, 46): (265, 67840), (PLANAR, 46): (265, 67840), (TORIC, 47): (277, 70912),
          (TORIC, 63): (497, 127232), (TORIC, 64): (512, 131072), (PLANAR, 64): (512, 131072)}
LIFT_SHAPES = [(TORIC, 45), (XZZX, 63), (ROTATED, 63), (TORIC, 46), (PLANAR, 46), (TORIC, 63), (TORIC, 64), (PLANAR, 64)]
# the class move needs logical lines of odd length on the torus: toric 46 / 64 are refused, 47 is the first toric shape through the opt-in
CORRECTION_SHAPES = [(TORIC, 45), (XZZX, 63), (ROTATED, 63), (TORIC, 47), (PLANAR, 46), (TORIC, 63), (PLANAR, 64)]
BYTE_SHAPES = [(TORIC, 33), (TORIC, 64), (PLANAR, 64), (XZZX, 63), (ROTATED, 63)]
NAMES = {TORIC: "toric", XZZX: "xzzx", ROTATED: "rotated", PLANAR: "planar"}


def shape_id(shape):
    return "%s-%d" % (NAMES[shape[0]], shape[1])


def ids(shapes):
    return [shape_id(s) for s in shapes]


def nq_of(code, L):
    return int(np.prod(state_shape(code, L)))


def on_branch(T, code, L):
    """W and the LDS bytes of a shape from the twin's lift table (its rows are W + 1 words), checked against BRANCH -> True iff the launch needs the opt-in"""
    words = -T.qt_lift_table(code, L, np.zeros(1, np.uint32).ctypes.data_as(_u32p), 0)      # (too small a buffer: minus the size)
    assert words > 0 and words % n_cells(code, L) == 0
    W = words // n_cells(code, L) - 1
    assert W == (nq_of(code, L) + 15) // 16
    assert (W, W * 64 * 4) == BRANCH[code, L], (W, W * 256)
    return W * 256 > DEFAULT_WINDOW


# ------------------------------------------------------------------------------------------------------------------ generators by their sites
@functools.lru_cache(maxsize=None)
def generator_sites(code, L):
    """(sites int32[n_gen, 4], paulis uint8[n_gen, 4]) of every generator in table order, from the oracle's stencil on the zero chain; a half
    plaquette's two missing sites have Pauli 0 (and site 0)"""
    zero = np.zeros(state_shape(code, L), dtype=np.uint8)
    if code == TORIC:
        args = [(r, c, op) for op in (1, 3) for r in range(L) for c in range(L)]
        apply = orc.toric_apply_stabilizer
    else:
        oc = ORC_CODE[code]
        args = [orc.surf_gen_rco(oc, L, g) for g in range(orc.surf_ngen(oc, L))]
        apply = lambda m, r, c, op: orc.surf_apply_stabilizer(oc, m, r, c, op)
    sites, paulis = np.zeros((len(args), 4), np.int32), np.zeros((len(args), 4), np.uint8)
    for g, a in enumerate(args):
        flat = apply(zero, *a)[0].ravel()
        at = np.flatnonzero(flat)
        assert 2 <= at.size <= 4
        sites[g, :at.size], paulis[g, :at.size] = at, flat[at]
    sites.setflags(write=False)
    paulis.setflags(write=False)
    return sites, paulis


def generator_changes(code, L, chains):
    """int[N, n_gen]: what applying each generator would do to the error count of each chain"""
    sites, paulis = generator_sites(code, L)
    f = np.asarray(chains).reshape(len(chains), -1)[:, sites]                               # [N, n_gen, 4]
    P = paulis[None]
    return np.where(P == 0, 0, np.where(f == 0, 1, np.where(f == P, -1, 0))).sum(axis=2)


def times_generators(code, L, m, gens):
    """the chain m times the generators with these indices"""
    sites, paulis = generator_sites(code, L)
    out = np.array(m, dtype=np.uint8)
    flat = out.reshape(-1)
    for g in gens:
        live = paulis[g] != 0
        flat[sites[g][live]] ^= paulis[g][live]
    return out


# ------------------------------------------------------------------------------------------------------------------ the lift
@functools.lru_cache(maxsize=None)
def lift_case(code, L):
    """70 random errors of a shape and their oracle syndromes with two rows made no syndromes of the code, as tests/test_gpu_syndrome_lift.py makes
    them (rows 10 and 66: one in each wavefront; every defect pattern of the planar code is a syndrome), and the twin's lift of them without
    and with the descent: dict(defects, bad, plain, low) with plain / low = (chains, status, weight).  Computed once, read-only."""
    T = lift_cpu.load_twin()
    _, d = lift_cpu.batch(code, L, n=N, seed=2)
    bad = []
    if code == TORIC:
        d[10, 3] ^= 1                                                 # an odd number of defects in a component of the torus
        d[66, L * L + 1] ^= 1
        bad = [10, 66]
    elif code != PLANAR:
        d[10, 0] = 1                                                  # corners of the (L+1)^2 grid are no checks
        d[66, (L + 1) * (L + 1) - 1] = 1
        bad = [10, 66]
    c = dict(defects=d, bad=np.array(bad, dtype=np.int64), plain=lift_cpu.twin(T, code, L, d, 0), low=lift_cpu.twin(T, code, L, d, 1))
    for v in (c["defects"], c["bad"]) + c["plain"] + c["low"]:
        v.setflags(write=False)
    return c


def small_lift(code, L, n):
    """n syndromes of a small shape and their twin lift with the descent (the rungs of the order test between the large ones)"""
    T = lift_cpu.load_twin()
    _, d = lift_cpu.batch(code, L, n=n, seed=2)
    return d, lift_cpu.twin(T, code, L, d, 1)


# ------------------------------------------------------------------------------------------------------------------ the corrections
KEYS = ("corrections", "weight", "source", "moved", "status")
BAD = {10: -1, 33: 1000, 66: None}                                    # out-of-range targets (None: ncls), as tests/test_gpu_corrections.py has them


@functools.lru_cache(maxsize=None)
def correction_case(code, L):
    """Errors of the oracle at p = 0.10 -- 5 on the torus, 18 elsewhere -- every one towards every target class (row s * ncls + t: error s
    towards class t), three candidates a row: the twin's lift of the error's syndrome, the error itself, and the lift with a logical operator
    somewhere and three generators on top.  80 or 72 rows.  Computed once, read-only."""
    T = corr_cpu.load_twin()
    n = corr_cpu.ncls_of(code)
    n_err = 5 if code == TORIC else 18
    rng = np.random.default_rng([9, code, L])
    _, raw, eq = orc.generate_syndromes(ORC_CODE[code], L, n_err, 0.1 / 3, 0.1 / 3, 0.1 / 3, hide_class=False, seed=7)
    defects = corr_cpu.syndromes(code, raw)
    lifted, status, _ = lift_cpu.twin(T, code, L, defects, 1)
    assert not status.any()
    third = np.empty_like(lifted)
    n_gen = len(generator_sites(code, L)[0])
    for s in range(n_err):
        m = corr_cpu.apply_kind(code, lifted[s], int(rng.integers(4 if code == TORIC else 2)), int(rng.integers(L)))
        third[s] = times_generators(code, L, m, rng.integers(n_gen, size=3))
    cand = np.stack([lifted, raw, third], axis=1)                                           # [n_err, 3, ...]
    flat = cand.reshape((n_err * 3,) + cand.shape[2:])
    assert np.array_equal(corr_cpu.syndromes(code, flat).reshape(n_err, 3, -1), np.repeat(defects[:, None], 3, axis=1))
    c = dict(errors=np.repeat(raw, n, axis=0), err_class=np.repeat(eq, n), defects=np.repeat(defects, n, axis=0), cand=np.repeat(cand, n, axis=0),
             cand_class=np.repeat(corr_cpu.classes(code, flat).reshape(n_err, 3), n, axis=0),
             cand_weight=np.repeat(corr_cpu.weights(flat).reshape(n_err, 3), n, axis=0), target=np.tile(np.arange(n, dtype=np.int32), n_err))
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def correction_batch(code, L, K):
    """the first 70 rows of correction_case with K of its candidates and three targets outside [0, ncls) -> (cand [70, K, ...], target)"""
    c = correction_case(code, L)
    cand, target = np.array(c["cand"][:N, :K]), np.array(c["target"][:N])
    for s, t in BAD.items():
        target[s] = corr_cpu.ncls_of(code) if t is None else t
    cand.setflags(write=False)
    target.setflags(write=False)
    return cand, target


@functools.lru_cache(maxsize=None)
def correction_twin(code, L, K, place, descend):
    cand, target = correction_batch(code, L, K)
    got = corr_cpu.twin(corr_cpu.load_twin(), code, L, cand, target, place, descend)
    for v in got.values():
        v.setflags(write=False)
    return got


def same(got, want):
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
