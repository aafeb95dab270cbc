"""A geometry-free sector law for (min, +, count): the least cost of a chain's class and the number of chains that reach it under costs with
c_I = 0 and c_Y = c_X + c_Z, from the oracle's stencils alone -- tests/util_sectors.py in the semiring of tests/util_minplus.py.

Under such costs the cost of a chain is a sum over its 2 nq symplectic bits: c_X for every set x bit, c_Z for every set z bit.  The generators fall
into sectors that share no bit (util_sectors.sectors), the bits of different sectors move independently, and a minimum of a sum of independent terms
is the sum of the minima: cost = the sum over the sectors of the sector's least cost, plus c_X / c_Z for every chain bit no generator acts on; the
subsets of the generators that reach it are the products of the sectors' minimisers, so their number is the product of the per-sector counts, and
every chain is met 2^(G - rank) times.  A sector never owns both bits of one qubit, so its generators and the chain's projection on its bits are
chains of {I, X} or {I, Z} per qubit and util_minplus.eliminate_minplus takes them unchanged, over a frontier of about half the full one.  Counts are
Python integers: nothing saturates here."""
import numpy as np

from util_minplus import eliminate_minplus
from util_sectors import bit_rows, gf2_rank, sectors


def sector_minplus(gens, chain, costs, order=None, parts=None, rank=None):
    """(cost, count) of the chain's class under costs = (0, c_X, c_X + c_Z, c_Z): the least cost over chain * the stabilizer group and the number of
    group elements that reach it, a Python integer.  parts = sectors(gens) and rank = gf2_rank(bit_rows(gens)) may be passed in where many chains
    share one table."""
    gens = np.asarray(gens, dtype=np.uint8)
    n_gen, nq = gens.shape
    c_i, c_x, c_y, c_z = (int(c) for c in costs)
    assert c_i == 0 and c_y == c_x + c_z, "the sector law needs c_I = 0 and c_Y = c_X + c_Z"
    parts = sectors(gens) if parts is None else parts
    rank = gf2_rank(bit_rows(gens)) if rank is None else rank
    have = bit_rows(np.asarray(chain, dtype=np.uint8).reshape(nq))
    cost, count, owned = 0, 1, np.zeros(2 * nq, dtype=bool)
    for idx, own in parts:
        owned |= own
        mine = have & own                                                       # the chain on this sector's bits: X where it owns x, Z where it owns z
        proj = (mine[:nq] * 1 + mine[nq:] * 3).astype(np.uint8)
        assert not np.any(gens[idx] == 2)                                       # (a Y would own both bits of its qubit)
        least, subsets = eliminate_minplus(gens[idx], proj, (0, c_x, c_y, c_z), order)
        cost, count = cost + least, count * subsets
    free = have & ~owned
    cost += c_x * int(free[:nq].sum()) + c_z * int(free[nq:].sum())
    assert count % (1 << (n_gen - rank)) == 0
    return cost, count >> (n_gen - rank)
