"""tests/util_minplus.py and tests/util_minplus_trace.py restated with a cost row per qubit: the (min, +, count) elimination over the oracle's stencils
and the brute force over the whole group, for the site costs of csrc/class_minplus_site.hpp.  Nothing here knows the planner, the op stream, the
packed cost words or the tie rule.  cq is an integer array [nq, 4]: the costs of I, X, Y and Z at every cell; only the cells a generator touches
enter."""
import numpy as np

from util_minplus import _forget
from util_minplus_trace import coset, qubit_cells


def eliminate_minplus(gens, chain, cq, order=None, max_axes=16):
    """(cost, count): over the subsets of the generators (byte chains [G, nq]) the least sum over the qubits of cq[q, chain_q ^ the generators of the
    subset at q], and the number of subsets that reach it, a Python integer -- 2^(G - rank) times the number of chains.  By variable elimination over
    the qubits in `order` (default: REVERSED)."""
    gens = np.asarray(gens)
    cq = np.asarray(cq, dtype=np.int64)
    n_gen, nq = gens.shape
    assert cq.shape == (nq, 4)
    left = (gens != 0).sum(axis=1)
    axes, cost, count = [], np.zeros((), np.int64), np.array(1, dtype=object)
    for q in (range(nq - 1, -1, -1) if order is None else order):
        here = [g for g in range(n_gen) if gens[g, q]]
        if not here:
            continue
        for g in here:
            if g not in axes:
                axes.append(g)
                cost, count = np.stack([cost, cost], axis=-1), np.stack([count, count], axis=-1)
        pauli = np.full((2,) * len(here), int(chain[q]))
        for i, g in enumerate(here):
            sel = np.arange(2).reshape([2 if j == i else 1 for j in range(len(here))])
            pauli = pauli ^ (sel * int(gens[g, q]))                             # (byte values XOR as the Pauli product)
        where = [axes.index(g) for g in here]
        shape = [1] * len(axes)
        for a in where:
            shape[a] = 2
        cost = cost + cq[q][pauli].transpose(np.argsort(where)).reshape(shape)
        count = np.broadcast_to(count, cost.shape)
        for g in here:
            left[g] -= 1
            if left[g] == 0:
                a = axes.index(g)
                cost, count = _forget(cost, count, a)
                axes.pop(a)
        assert len(axes) <= max_axes, "the order of this test opens too many generators at once"
    assert not axes
    return int(cost), int(count)


def site_cost(gens, chain, cq):
    """the sum of cq[q, Pauli at q] over the cells that hold a qubit"""
    chain = np.asarray(chain, dtype=np.uint8).ravel()
    cells = np.flatnonzero(qubit_cells(gens))
    return int(np.asarray(cq, dtype=np.int64).reshape(-1, 4)[cells, chain[cells]].sum())


def brute_force_minplus(gens, chain, cq, chains=None):
    """(cost, the number of subsets that reach it, the DISTINCT chains that reach it uint8[k, nq]) over coset(gens, chain): the definition"""
    chains = coset(gens, chain) if chains is None else chains
    cells = np.flatnonzero(qubit_cells(gens))
    costs = np.asarray(cq, dtype=np.int64).reshape(-1, 4)[cells[None, :], chains[:, cells]].sum(axis=1)
    return int(costs.min()), int((costs == costs.min()).sum()), np.unique(chains[costs == costs.min()], axis=0)


def brute_force_max_product(gens, chain, wq, chains=None):
    """the DISTINCT chains of coset(gens, chain) with the largest product over the qubits of wq[q, Pauli at q] (float [nq, 4]), compared in exact
    rational arithmetic where the weights are given as Fractions, in float64 otherwise"""
    chains = coset(gens, chain) if chains is None else chains
    cells = np.flatnonzero(qubit_cells(gens))
    wq = np.asarray(wq, dtype=object).reshape(-1, 4)
    prods = [np.prod(wq[cells, row[cells]]) for row in chains]
    best = max(prods)
    return np.unique(chains[[i for i, v in enumerate(prods) if v == best]], axis=0)
