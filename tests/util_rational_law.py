"""The class law in exact rational arithmetic: what the sum-product sweeps and the law functions of qecmc.exact are held to at the ends of float64's
range, where a float64 reference has no digits left to compare with.  Fraction(float) is exact, so the reference sees the very weights a sweep is
given.  Nothing of the sweeps' planner or of their twins is used here.

Two forms.  Uniform weights: the integer class histogram of a syndrome over (n_xy, n_z) -- from the enumerator's twin, or from
util_exact.SurfEnumeration -- summed against powers of the two weights.  Site weights: a brute force over every subset of the oracle's generator
stencils (rank <= 12: xzzx, rotated and planar L = 3), products and sums in Fractions.  The toric code at L = 3 (2^16 x 16 chains) is covered through
the histogram form only."""
from fractions import Fraction

import numpy as np

TINY = Fraction(1, 2 ** 1074)                                                   # the least positive double
FLOOR = Fraction(1, 2 ** 960)                                                   # below this total the law functions may refuse, at or above it they may not


def dyadic(x):
    """(m, e) with float x == m / 2^e exactly, m an int"""
    fr = Fraction(float(x))
    e = fr.denominator.bit_length() - 1
    assert fr.denominator == 1 << e
    return fr.numerator, e


def uniform_class_weights(hist, w_xy, w_z):
    """[Fraction] * ncls: Z_c = the sum over (i, j) of hist[c, i, j] * w_xy^i * w_z^j exactly, for floats w_xy (the weight of X and of Y) and w_z, in the
    ratio form the sweeps use (the weight of I is 1).  The terms are summed over their common power-of-two denominator -- what Fraction would do,
    without a gcd at every step."""
    hist = np.asarray(hist)
    (a, ea), (b, eb) = dyadic(w_xy), dyadic(w_z)
    n = hist.shape[-1]
    if (a, ea) == (b, eb):                                                      # one weight for X, Y and Z: fold the counts onto n_xy + n_z first
        num = [[sum(int(h[i, k - i]) for i in range(max(0, k - n + 1), min(k, n - 1) + 1)) for k in range(2 * n - 1)] for h in hist]
        pa, depth = [a ** k for k in range(2 * n - 1)], ea * (2 * n - 2)
        return [Fraction(sum((c * pa[k]) << (depth - ea * k) for k, c in enumerate(row) if c), 1 << depth) for row in num]
    pa, pb = [a ** i for i in range(n)], [b ** j for j in range(n)]
    depth = (ea + eb) * (n - 1)
    out = []
    for h in hist:
        num = 0
        for i, j in zip(*np.nonzero(h)):
            i, j = int(i), int(j)
            num += (int(h[i, j]) * pa[i] * pb[j]) << (depth - ea * i - eb * j)
        out.append(Fraction(num, 1 << depth))
    return out


def law(z):
    """[Fraction]: z normalised (the exact class law)"""
    total = sum(z)
    return [x / total for x in z]


def least_cost_and_count(hist):
    """[(cost, count)] * ncls under unit costs: the least n_xy + n_z with a chain of the class, and the number of chains that have it"""
    out = []
    for h in np.asarray(hist):
        i, j = np.nonzero(h)
        least = int((i + j).min())
        out.append((least, int(sum(int(h[a, b]) for a, b in zip(i, j) if a + b == least))))
    return out


def group_of(gens):
    """every product of a subset of the generators (byte chains uint8[G, nq]: byte values XOR as the Pauli product) once: uint8[2^rank, nq]"""
    grp = np.zeros((1, gens.shape[1]), np.uint8)
    for g in np.asarray(gens, dtype=np.uint8):
        grp = np.concatenate([grp, grp ^ g])
    return np.unique(grp, axis=0)


def site_class_weights(gens, reps, wq):
    """[Fraction] * ncls: Z_c = the sum over the stabilizer group of the product over the qubits a generator touches of wq[q][Pauli of (reps[c] times the
    group element) at q], exactly.  gens uint8[G, nq]: the oracle's stencils; reps uint8[ncls, nq]: one chain per class; wq float[nq, 4]."""
    gens = np.asarray(gens, dtype=np.uint8)
    assert len(gens) <= 12, "the brute force is meant for L = 3"
    touched = np.flatnonzero(gens.any(axis=0))
    w = {(int(q), k): Fraction(float(wq[q][k])) for q in touched for k in range(4)}
    grp = group_of(gens)
    out = []
    for rep in np.asarray(reps, dtype=np.uint8):
        total = Fraction(0)
        for chain in (grp ^ rep)[:, touched].tolist():
            term = Fraction(1)
            for q, k in zip(touched.tolist(), chain):
                term *= w[q, k]
                if not term:
                    break
            total += term
        out.append(total)
    return out


def close_to(got, want, rel):
    """|got - want| <= rel * want for a float got and a Fraction want > 0, exactly"""
    return abs(Fraction(float(got)) - want) <= Fraction(rel) * want
