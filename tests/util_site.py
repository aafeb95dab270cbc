"""An elimination under site weights that knows nothing of the planner: tests/test_class_sweep_cpu.eliminate with the factor of a qubit read from that
qubit's own row of a weight table, over the oracle's stencils."""
import numpy as np


def eliminate_site(gens, chain, wq, order=None):
    """sum over the subsets of the generators (byte chains [G, nq], the oracle's stencils) of prod_q wq[q][chain_q ^ the generators of the subset at q]
    -- wq float[nq, 4], the weights of I, X, Y, Z at every qubit -- by variable elimination over the qubits in `order` (default: REVERSED): a NumPy
    array with one axis per open generator.  Every group element is met 2^(G - rank) times, as in eliminate."""
    gens = np.asarray(gens)
    wq = np.asarray(wq, dtype=np.float64)
    n_gen, nq = gens.shape
    assert wq.shape == (nq, 4)
    left = (gens != 0).sum(axis=1)
    axes, A = [], np.ones(())
    for q in (range(nq - 1, -1, -1) if order is None else order):
        here = [g for g in range(n_gen) if gens[g, q]]
        if not here:
            continue
        for g in here:
            if g not in axes:
                axes.append(g)
                A = np.stack([A, A], axis=-1)
        pauli = np.full((2,) * len(here), int(chain[q]))
        for i, g in enumerate(here):
            sel = np.arange(2).reshape([2 if j == i else 1 for j in range(len(here))])
            pauli = pauli ^ (sel * int(gens[g, q]))                             # (byte values XOR as the Pauli product)
        factor = wq[q][pauli]
        where = [axes.index(g) for g in here]
        shape = [1] * len(axes)
        for i, a in enumerate(where):
            shape[a] = 2
        A = A * factor.transpose(np.argsort(where)).reshape(shape)
        for g in here:
            left[g] -= 1
            if left[g] == 0:
                a = axes.index(g)
                A = A.sum(axis=a)
                axes.pop(a)
        assert len(axes) <= 16, "the order of this test opens too many generators at once"
    assert not axes
    return float(A)


def random_site_weights(rng, shape):
    """weights drawn log-uniformly in [1e-3, 1]: float64[shape + (4,)]"""
    return np.exp(rng.uniform(np.log(1e-3), 0.0, size=tuple(shape) + (4,)))
