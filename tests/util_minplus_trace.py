"""tests/util_minplus.py's brute force with the chains kept: the argmin of the enumeration, for the traceback of csrc/class_minplus_trace.hpp.  Nothing
here knows the planner, the op stream or the tie rule."""
import numpy as np


def qubit_cells(gens):
    """bool[nq]: the cells a generator touches -- the cells that hold a qubit"""
    return np.asarray(gens).any(axis=0)


def chain_cost(gens, chain, cost4):
    """the sum of cost4[Pauli] over the cells that hold a qubit"""
    chain = np.asarray(chain, dtype=np.uint8).ravel()
    return int(np.asarray(cost4, dtype=np.int64)[chain[qubit_cells(gens)]].sum())


def coset(gens, chain):
    """every subset of the generators (G <= 20) applied to the chain: uint8[2^G, nq]"""
    gens = np.asarray(gens, dtype=np.uint8)
    assert len(gens) <= 20
    chains = np.asarray(chain, dtype=np.uint8).reshape(1, -1)
    for g in gens:
        chains = np.concatenate([chains, chains ^ g])
    return chains


def brute_force_argmin(gens, chain, cost4, chains=None):
    """(cost, number of DISTINCT chains that reach it, those chains uint8[k, nq]) over coset(gens, chain) -- which a caller with several cost vectors
    passes in --: the definition.  Dependent generators give every chain several times, so the chains are made unique before they are counted."""
    chains = coset(gens, chain) if chains is None else chains
    costs = np.asarray(cost4, dtype=np.int64)[chains[:, qubit_cells(gens)]].sum(axis=1)
    best = np.unique(chains[costs == costs.min()], axis=0)
    return int(costs.min()), len(best), best
