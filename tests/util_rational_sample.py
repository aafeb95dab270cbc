"""The law of a chain and the marginals of a class in exact rational arithmetic: what the exact chain sampler (csrc/class_sample.hpp) and the exact
marginals (csrc/class_marginal.hpp) are held to at the ends of float64's range, beside util_rational_law.py.  Nothing of the sweeps' planner, of the
record, of the walk or of their twins is used here: a coset is the oracle's stencils times a representative, a chain's weight the product of its
factors, and every float is taken for the dyadic rational it is.

A weight is kept as an integer numerator over a power of two -- a float is m / 2^e exactly --, so the products and sums below are integer products
and sums over one common denominator per coset, with no gcd on the way; Fractions are formed where a caller asks for one."""
from fractions import Fraction

import numpy as np

from util_rational_law import dyadic, group_of


def touched_cells(gens):
    """the cells some generator touches, ascending: the qubits a chain's weight runs over"""
    return np.flatnonzero(np.asarray(gens).any(axis=0))


def coset_of(gens, rep):
    """uint8[2^rank, nq]: every chain of the class of `rep`, once, sorted as np.unique sorts rows"""
    return np.unique(group_of(gens) ^ np.asarray(rep, dtype=np.uint8).ravel(), axis=0)


class Weights:
    """four weights float[4] (I, X, Y, Z) or a site table float[nq, 4], as dyadic rationals per (cell, Pauli)"""

    def __init__(self, gens, w):
        w = np.asarray(w, dtype=np.float64)
        self.cells = [int(q) for q in touched_cells(gens)]
        self.table = [[dyadic(w[k] if w.ndim == 1 else w[q, k]) for k in range(4)] for q in self.cells]
        self.depth = sum(max(e for _, e in row) for row in self.table)          # every chain's weight is an integer over 2^depth

    def numerator(self, chain):
        """the weight of a chain (uint8[nq], or the list of its bytes) times 2^depth, an int"""
        num, exp = 1, 0
        for row, q in zip(self.table, self.cells):
            m, e = row[chain[q]]
            if not m:
                return 0
            num *= m
            exp += e
        return num << (self.depth - exp)

    def weight(self, chain):
        """Fraction: the product over the touched cells of w[Pauli of the chain there]"""
        return Fraction(self.numerator(chain), 1 << self.depth)


class CosetLaw:
    """one class under one set of weights: chains uint8[n, nq] (sorted), num [int] * n with w(chain) = num / 2^depth, total = their sum"""

    def __init__(self, gens, rep, w, coset=None):
        self.weights = w if isinstance(w, Weights) else Weights(gens, w)
        self.chains = coset_of(gens, rep) if coset is None else coset
        self.num = [self.weights.numerator(c) for c in self.chains.tolist()]
        self.total = sum(self.num)
        self.depth = self.weights.depth

    @property
    def z(self):
        """Fraction: Z_c"""
        return Fraction(self.total, 1 << self.depth)

    def law(self):
        """[Fraction]: w(chain) / Z_c in the order of chains"""
        return [Fraction(n, self.total) for n in self.num]

    def index(self):
        """dict: the bytes of a chain -> its row"""
        return {c.tobytes(): i for i, c in enumerate(self.chains)}

    def marginal_numerators(self):
        """[nq][4] ints: the sum of num over the chains that carry Pauli P at q -- weights[c, q, P] of the marginals times 2^depth"""
        if getattr(self, "_marginal", None) is not None:
            return self._marginal
        nq = self.chains.shape[1]
        out = [[0, 0, 0, 0] for _ in range(nq)]
        for chain, n in zip(self.chains.tolist(), self.num):
            if n:
                for q, k in enumerate(chain):
                    out[q][k] += n
        return out

    def marginals(self):
        """[nq][4] Fractions: P(q carries P | syndrome, class)"""
        return [[Fraction(x, self.total) for x in row] for row in self.marginal_numerators()]


class UniformCoset:
    """a coset under weights (1, f, f, f), for many f: the chains' error counts over the touched cells and, per (cell, Pauli, error count), the number
    of chains -- counted once; at(f) is then the CosetLaw of f without another pass over the chains"""

    def __init__(self, gens, coset):
        self.cells = [int(q) for q in touched_cells(gens)]
        self.chains = coset
        self.k = np.count_nonzero(coset[:, self.cells], axis=1).tolist()
        nq, top = coset.shape[1], len(self.cells) + 1
        self.table = [[[0] * top for _ in range(4)] for _ in range(nq)]
        for chain, k in zip(coset.tolist(), self.k):
            for q, P in enumerate(chain):
                self.table[q][P][k] += 1

    def at(self, f):
        m, e = dyadic(f)
        n = len(self.cells)
        power = [m ** k << (e * (n - k)) for k in range(n + 1)]              # f^k over 2^(e n)
        law = CosetLaw.__new__(CosetLaw)
        law.weights, law.chains, law.depth = None, self.chains, e * n
        law.num = [power[k] for k in self.k]
        law.total = sum(law.num)
        law._marginal = [[sum(c * pw for c, pw in zip(row, power) if c) for row in cell] for cell in self.table]
        return law


def posterior_marginals(laws):
    """[nq][4] Fractions: P(q carries P | syndrome) from the CosetLaws of every class of one syndrome under one set of weights"""
    depth = laws[0].depth
    assert all(x.depth == depth for x in laws)
    total = sum(x.total for x in laws)
    per = [x.marginal_numerators() for x in laws]
    return [[Fraction(sum(p[q][k] for p in per), total) for k in range(4)] for q in range(len(per[0]))]


def error_count(marginals, cells):
    """Fraction: sum over the cells that hold a qubit of 1 - P(I)"""
    return sum(1 - marginals[q][0] for q in cells)


def one_chain_table(gens, chain, scale_total, rng=None):
    """A site table float64[nq, 4] under which exactly one chain of the whole syndrome has weight > 0: each touched cell gives the chain's Pauli one
    positive weight and the other three 0 (an untouched cell gets (1, 1, 1, 1): it carries no factor).  The positive weights are powers of two whose
    product is exactly scale_total -- a power of two down to 2^-1074 --, spread so that no single factor leaves the normal range."""
    chain = np.asarray(chain, dtype=np.uint8).ravel()
    cells = touched_cells(gens)
    m, e = dyadic(scale_total)
    assert m == 1, "a power of two"
    share = [e // len(cells) + (1 if i < e % len(cells) else 0) for i in range(len(cells))]
    out = np.ones((len(chain), 4))
    for q, k in zip(cells, share):
        out[q] = 0.0
        out[q, chain[q]] = 2.0 ** -k
    return out
