"""A (min, +, count) elimination that knows nothing of the planner: tests/test_class_sweep_cpu.eliminate in the semiring of (cost, count) pairs, over the
oracle's stencils.  The state is a pair of NumPy arrays with one axis per open generator: the least cost so far (int64) and the number of assignments
that reach it (dtype object: Python integers, which neither saturate nor overflow)."""
import numpy as np


def _forget(cost, count, axis):
    """fold one axis: the smaller cost; on a tie the counts add"""
    c0, c1 = np.take(cost, 0, axis=axis), np.take(cost, 1, axis=axis)
    n0, n1 = np.take(count, 0, axis=axis), np.take(count, 1, axis=axis)
    least = np.minimum(c0, c1)
    return least, np.where(c0 == least, n0, 0) + np.where(c1 == least, n1, 0)


def eliminate_minplus(gens, chain, cost4, order=None, max_axes=16):
    """(cost, count): over the subsets of the generators (byte chains [G, nq], the oracle's stencils) the least sum over the qubits of
    cost4[chain_q ^ the generators of the subset at q] -- cost4: the integer costs of I, X, Y, Z; only the qubits a generator touches enter -- and the
    number of subsets that reach it, a Python integer.  Every group element is met 2^(G - rank) times, so count is that multiple of the number of
    chains.  By variable elimination over the qubits in `order` (default: REVERSED)."""
    gens = np.asarray(gens)
    cost4 = np.asarray(cost4, dtype=np.int64)
    n_gen, nq = gens.shape
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
        cost = cost + cost4[pauli].transpose(np.argsort(where)).reshape(shape)
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


def brute_force_minplus(gens, chain, cost4):
    """eliminate_minplus by the definition: every subset of the generators (G <= 20), its chain, its cost over the qubits a generator touches"""
    gens = np.asarray(gens, dtype=np.uint8)
    assert len(gens) <= 20
    chains = np.asarray(chain, dtype=np.uint8).reshape(1, -1)
    for g in gens:
        chains = np.concatenate([chains, chains ^ g])
    touched = gens.any(axis=0)
    costs = np.asarray(cost4, dtype=np.int64)[chains[:, touched]].sum(axis=1)
    return int(costs.min()), int((costs == costs.min()).sum())
