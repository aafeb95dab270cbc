"""The sector product of tests/util_sectors.py under a weight per qubit: the class weight Z of a chain under a table whose rows are
w_q = c_q (1, fx_q, fx_q fz_q, fz_q), from the oracle's stencils alone.

The weight of a chain is then prod_q c_q times fx_q for every set x bit (q, x) and fz_q for every set z bit (q, z): it still factorises over the
2 nq symplectic bits, only with a factor of its own per bit.  So the split of util_sectors.sectors holds unchanged -- the sum over the 2^G subsets
of the generators is one sum per sector, times the factor of every chain bit no generator owns, times prod_q c_q, and every group element is met
2^(G - rank) times.  A sector never owns both bits of a qubit, so per sector util_site.eliminate_site sums the chain's projection under the rows
(1, fx_q, 0, fz_q).  Zero is a legal fx_q or fz_q: pure erasure is fx = fz = 1 on the erased cells and 0 elsewhere.

Cells that hold no qubit (the planar array's idle row and column) follow the twins' convention: they are never read, so c_q and the free-bit
factors run over the qubits some generator acts on alone, and such a cell may hold anything -- NaN included."""
import numpy as np

import util_sectors as U
from util_site import eliminate_site


def site_table(c, fx, fz):
    """the table of w_q = c_q (1, fx_q, fx_q fz_q, fz_q): float64[..., 4] in the order I, X, Y, Z"""
    c, fx, fz = np.broadcast_arrays(np.asarray(c, np.float64), np.asarray(fx, np.float64), np.asarray(fz, np.float64))
    return np.stack([c, c * fx, c * (fx * fz), c * fz], axis=-1)


def random_factors(rng, shape, erased=None, low=1e-2):
    """(c, fx, fz) float64[shape]: c uniform in [0.5, 1], fx and fz log-uniform in [low, 1]; on the cells of the bool mask `erased` c = fx = fz = 1,
    which is erasure_site_w4's (1, 1, 1, 1)"""
    c = rng.uniform(0.5, 1.0, size=shape)
    fx, fz = np.exp(rng.uniform(np.log(low), 0.0, size=(2,) + tuple(shape)))
    if erased is not None:
        c[erased], fx[erased], fz[erased] = 1.0, 1.0, 1.0
    return c, fx, fz


def site_sector_product(gens, chain, c, fx, fz, order=None, parts=None, rank=None):
    """Z of the chain's class under w_q = c_q (1, fx_q, fx_q fz_q, fz_q), c, fx, fz float[nq]: the sum over the stabilizer group of the weight of
    chain * element.  parts = util_sectors.sectors(gens) and rank = gf2_rank(bit_rows(gens)) may be passed in where many chains share one table."""
    gens = np.asarray(gens, dtype=np.uint8)
    n_gen, nq = gens.shape
    c, fx, fz = (np.asarray(a, dtype=np.float64).reshape(nq) for a in (c, fx, fz))
    parts = U.sectors(gens) if parts is None else parts
    rank = U.gf2_rank(U.bit_rows(gens)) if rank is None else rank
    used = (gens != 0).any(axis=0)                                              # the qubits some generator acts on: the others are never read
    have = U.bit_rows(np.asarray(chain, dtype=np.uint8).reshape(nq))
    assert not have[np.concatenate([~used, ~used])].any(), "the chain acts on a cell that holds no qubit"
    rows = np.zeros((nq, 4))
    rows[used] = np.stack([np.ones(int(used.sum())), fx[used], np.zeros(int(used.sum())), fz[used]], axis=-1)
    z, owned = 1.0, np.zeros(2 * nq, dtype=bool)
    for idx, own in parts:
        owned |= own
        mine = have & own                                                       # the chain on this sector's bits: X where it owns x, Z where it owns z
        proj = (mine[:nq] * 1 + mine[nq:] * 3).astype(np.uint8)
        assert not np.any(gens[idx] == 2)                                       # (a Y would own both bits of its qubit)
        z *= eliminate_site(gens[idx], proj, rows, order)
    free = have & ~owned                                                        # on a used qubit: a bit of it that no generator moves
    z *= np.prod(fx[free[:nq]]) * np.prod(fz[free[nq:]])
    return z * np.prod(c[used]) * 0.5 ** (n_gen - rank)
