"""A geometry-free sector product: the class weight Z of a chain under weights with w_Y = w_X w_Z, from the oracle's stencils alone.

With w = (1, fx, fx fz, fz) the weight of a chain factorises over its 2 nq symplectic bits -- fx for every set x bit (q, x), fz for every set z bit
(q, z).  Link two generators when they act on a common bit: the table falls into components (sectors), the bits of different sectors move
independently, and the sum over all 2^G subsets of the generators is the product of one sum per sector, times fx / fz for every chain bit no
generator acts on.  Every group element is met 2^(G - rank) times.  A sector never owns both bits of one qubit (asserted), so its generators and
the chain's projection on its bits are chains of {I, X} or {I, Z} per qubit and test_class_sweep_cpu.eliminate sums them unchanged with
w4 = (1, fx, 0, fz): a frontier of about half the full one.  The rank is a GF(2) elimination written here.  On the torus the sectors are "all X" and
"all Z"; for xzzx they are two mixed X / Z checkerboards."""
import numpy as np

import test_class_sweep_cpu as cpu
from test_syndrome_lift_cpu import PLANAR, TORIC


def bit_rows(chains):
    """byte chains [..., nq] (1 = X, 2 = Y, 3 = Z) as symplectic bits bool[..., 2 nq]: bit q is (q, x), bit nq + q is (q, z)"""
    chains = np.asarray(chains)
    return np.concatenate([(chains == 1) | (chains == 2), chains >= 2], axis=-1)


def sectors(gens):
    """the components of the generators uint8[G, nq] linked through a shared symplectic bit: a list of (generator indices, the bits they act on as
    bool[2 nq]), in the order of each component's first generator"""
    rows = bit_rows(gens)
    n_gen, nq = gens.shape
    parent = list(range(2 * nq))

    def find(b):
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        return b

    for r in rows:
        mine = np.flatnonzero(r)
        assert len(mine), "a generator that acts on nothing"
        for b in mine[1:]:
            parent[find(int(b))] = find(int(mine[0]))
    members = {}
    for g, r in enumerate(rows):
        members.setdefault(find(int(np.flatnonzero(r)[0])), []).append(g)
    out = []
    for idx in members.values():
        own = rows[idx].any(axis=0)
        assert not (own[:nq] & own[nq:]).any(), "a sector owns the x and the z bit of one qubit"
        out.append((np.array(idx), own))
    assert sum(len(idx) for idx, _ in out) == n_gen and np.sum([own for _, own in out], axis=0).max() == 1     # a partition of the table, disjoint bits
    return out


def gf2_rank(rows):
    """the rank of a bit matrix bool[G, n] over GF(2), by elimination on Python integers"""
    rank, pivots = 0, []
    for r in np.asarray(rows, dtype=bool):
        v = sum(1 << int(b) for b in np.flatnonzero(r))
        for p in pivots:
            v = min(v, v ^ p)
        if v:
            pivots.append(v)
            pivots.sort(reverse=True)
            rank += 1
    return rank


def order_for(code, L):
    """the qubit order in which eliminate keeps its frontier within 16 generators: reversed index (None) for rotated / xzzx, column by column for
    planar, row by row of the lattice in half steps for toric"""
    if code == PLANAR:
        return cpu.column_major(code, L)
    if code == TORIC:
        return torus_order(L)
    return None


def torus_order(L):
    """the torus' qubits row by row of the lattice in half steps (layer 1 holds the horizontal edges of a row, layer 0 the vertical ones below it), last
    row first (as tests/test_gpu_class_sweep_tiled.py has it)"""
    key = lambda q: (2 * (q % (L * L) // L) + (0 if q >= L * L else 1), 2 * (q % L) + (1 if q >= L * L else 0))
    return sorted(range(2 * L * L), key=key, reverse=True)


def sector_product(gens, chain, fx, fz, order=None, parts=None, rank=None):
    """Z of the chain's class under w = (1, fx, fx fz, fz): the sum over the stabilizer group of the weight of chain * element.  parts = sectors(gens)
    and rank = gf2_rank(bit_rows(gens)) may be passed in where many chains share one table."""
    gens = np.asarray(gens, dtype=np.uint8)
    n_gen, nq = gens.shape
    parts = sectors(gens) if parts is None else parts
    rank = gf2_rank(bit_rows(gens)) if rank is None else rank
    have = bit_rows(np.asarray(chain, dtype=np.uint8).reshape(nq))
    w4 = np.array([1.0, fx, 0.0, fz])
    z, owned = 1.0, np.zeros(2 * nq, dtype=bool)
    for idx, own in parts:
        owned |= own
        mine = have & own                                                       # the chain on this sector's bits: X where it owns x, Z where it owns z
        proj = (mine[:nq] * 1 + mine[nq:] * 3).astype(np.uint8)
        assert not np.any(gens[idx] == 2)                                       # (a Y would own both bits of its qubit)
        z *= cpu.eliminate(gens[idx], proj, w4, order)
    free = have & ~owned
    z *= fx ** int(free[:nq].sum()) * fz ** int(free[nq:].sum())
    return z * 0.5 ** (n_gen - rank)
