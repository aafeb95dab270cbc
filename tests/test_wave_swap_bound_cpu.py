"""The swap sweep's bound of the scan = "wave" kernels (csrc/wu_bounds.hpp).  Slots i and i + 1 trade states iff d <= 0 or x < swap_thr[i][d] with d the
difference of their error counts (mcmc.py:146-149); the thresholds fall with d, so whoever draws x can leave D_i(x), the largest d in [0, nq] with d == 0 or
x < swap_thr[i][d], and the cascade tests d <= D_i(x) without a table.  The bound is a host-callable inline function: it runs here through the plain
tables library (g++ alone, no HIP, no GPU) on the plans' own tables, for every pair, and must equal the brute-force maximum whatever its log2 guess says --
at every threshold and its two neighbours, at 0, 1, 2 (where the thresholds have saturated at 1 and the answer is nq: the table walk) and 2^32 - 1, and
on seeded words -- and d <= bound must be the old rule for every d in [-nq, nq]."""
import ctypes as C

import numpy as np
import pytest

from hostlib import tables_lib
from qecmc import _lib as L_

PLANS = [  # L, p, Nc (toric)
    pytest.param(9, 0.15, 8, id="config2"),
    pytest.param(5, 0.10, 5, id="L5-Nc5"),
    pytest.param(9, 0.15, 16, id="L9-Nc16"),
    pytest.param(9, 0.05, 2, id="L9-Nc2"),
    pytest.param(11, 0.18, 8, id="L11-Nc8"),
]


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_wave_swap_bound.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.qt_wave_swap_row.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


def _params(L, p, Nc):
    return L_.make_params(code=L_.TORIC, L=L, Nc=Nc, p=p, p_logical=0.5, iters=10, steps=10, scan=L_.SCAN_WAVE)


def _row(T, pr, pair, nq):
    row = np.zeros(nq + 1, np.uint64)
    assert T.qt_wave_swap_row(C.byref(pr), pair, row.ctypes.data, row.size) == nq + 1
    return row


def _inputs(row, seed):
    """every threshold of d >= 1 and its two neighbours, the ends of the range, the saturated end, seeded words"""
    t = row[1:].astype(np.int64)
    xs = np.concatenate([t - 1, t, t + 1, np.array([0, 1, 2, 2**32 - 1], np.int64),
                         np.random.default_rng(seed).integers(0, 2**32, size=20000, dtype=np.int64)])
    return np.unique(xs[(xs >= 0) & (xs < 2**32)]).astype(np.uint32)


@pytest.mark.parametrize("L,p,Nc", PLANS)
def test_bound_is_the_largest_passing_distance_and_restates_the_rule(T, L, p, Nc):
    pr, nq = _params(L, p, Nc), 2 * L * L
    ds = np.arange(-nq, nq + 1)
    for pair in range(Nc - 1):
        row = _row(T, pr, pair, nq)
        assert (row[1:] <= 0xFFFFFFFF).all() and (np.diff(row[1:].astype(np.int64)) <= 0).all(), "the row falls with d and fits 32 bits"
        xs = _inputs(row, 1000 * L + 16 * Nc + pair)
        got = np.zeros(xs.size, np.uint32)
        assert T.qt_wave_swap_bound(C.byref(pr), pair, xs.ctypes.data, xs.size, got.ctypes.data) == nq
        # the brute force: x < row[d] holds for a prefix of d = 1 .. nq only if the row falls, which is not assumed here -- the largest d that passes
        passes = xs[:, None].astype(np.uint64) < row[None, 1:]                       # [x][d - 1]
        brute = np.where(passes.any(axis=1), nq - np.argmax(passes[:, ::-1], axis=1), 0)
        assert np.array_equal(got, brute.astype(np.uint32))
        assert row[nq] >= 1 and got[0] == nq and xs[0] == 0, "x = 0 lies below every threshold, saturated ones included: the table walk up to nq"
        # d <= bound against d <= 0 or x < row[d], for every d the records can give
        old = (ds[None, :] <= 0) | (xs[:, None].astype(np.uint64) < row[np.clip(ds, 0, nq)][None, :])
        new = ds[None, :] <= got[:, None].astype(np.int64)
        assert np.array_equal(new, old)

