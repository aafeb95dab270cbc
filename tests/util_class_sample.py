"""An independent brute force for the exact chain sampler (csrc/class_sample.hpp) at L = 3: the coset of every class enumerated with the oracle's
stencils, as tests/util_exact.py enumerates it, with every chain's w(chain) / Z_c; Pearson's chi-square against it; and the sampler's uniform
u53(block, j) restated in a few lines of numpy on the oracle's Philox.  Nothing here knows the planner, the op stream, the record or the walk."""
import itertools
import math

import numpy as np

from oracle import oracle as orc
from test_corrections_cpu import TORIC, apply_kind, generators, ncls_of, oracle_class
from test_syndrome_lift_cpu import state_shape
from util_minplus_trace import coset, qubit_cells

SUB_SAMPLE = 0x53                        # the sub-stream of every draw (DESIGN.md "RNG addressing")


def u53(seed, syndrome, stream, k, block, j):
    """the uniform of sample k at (block, j): words 2j and 2j + 1 of philox_block(k << 16 | block, SUB_SAMPLE, syndrome, stream, seed)"""
    index = (int(k) << 16) | int(block)
    ctr = [index & 0xFFFFFFFF, ((index >> 32) & 0xFFFF) | (SUB_SAMPLE << 16), int(syndrome) & 0xFFFFFFFF, int(stream)]
    w = orc.philox4x32_10(ctr, [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF])
    return float((w[2 * j] << 21) | (w[2 * j + 1] >> 11)) * 2.0 ** -53


def class_representatives(code, chain):
    """one chain of every class with the syndrome of `chain`, uint8[ncls, nq]: the chain times products of the oracle's logical operators"""
    shape = np.asarray(chain).shape
    L = shape[-1]
    kinds = 4 if code == TORIC else 2
    reps = {}
    for bits in itertools.product((0, 1), repeat=kinds):
        m = np.array(chain, dtype=np.uint8).reshape(state_shape(code, L))
        for kind, on in enumerate(bits):
            if on:
                m = np.asarray(apply_kind(code, m, kind), dtype=np.uint8)
        reps.setdefault(int(oracle_class(code, m)), m.ravel().copy())
    assert sorted(reps) == list(range(ncls_of(code)))
    return np.stack([reps[c] for c in range(ncls_of(code))])


def chain_weights(gens, chains, w):
    """float64[n]: the product over the cells that hold a qubit of w[Pauli] -- w float[4], or a table float[nq, 4]"""
    cells = np.flatnonzero(qubit_cells(gens))
    w = np.asarray(w, dtype=np.float64)
    chains = np.asarray(chains, dtype=np.uint8)[:, cells]
    factors = w[chains] if w.ndim == 1 else w[cells[None, :], chains]
    return factors.prod(axis=1)


def class_law(code, L, chain, w):
    """per class c: (the distinct chains of the class uint8[n_c, nq], their probabilities w(chain) / Z_c float64[n_c], Z_c) -- the definition"""
    gens = generators(code, L)
    out = []
    for rep in class_representatives(code, chain):
        chains = np.unique(coset(gens, rep), axis=0)
        wt = chain_weights(gens, chains, w)
        out.append((chains, wt / wt.sum(), float(wt.sum())))
    return out


def chi_square(counts, prob, min_expected=5.0):
    """Pearson's statistic of integer counts against probabilities and its degrees of freedom.  A count in a bin of probability 0 makes it infinite.
    Bins that expect fewer than min_expected samples are pooled, the least likely first, until the pool expects that many (what is left over joins
    the last pool): which bins are pooled is decided by prob and the number of samples alone, never by the counts"""
    counts, prob = np.asarray(counts, dtype=np.float64), np.asarray(prob, dtype=np.float64)
    if counts[prob == 0].any():
        return np.inf, 0
    order = np.argsort(prob[prob > 0], kind="stable")
    expect, got = (counts.sum() * prob[prob > 0])[order], counts[prob > 0][order]
    e_bins, g_bins, e, g = [], [], 0.0, 0.0
    for ei, gi in zip(expect, got):
        e, g = e + ei, g + gi
        if e >= min_expected:
            e_bins.append(e); g_bins.append(g)
            e, g = 0.0, 0.0
    if e > 0.0 and e_bins:
        e_bins[-1] += e; g_bins[-1] += g
    e_bins, g_bins = np.array(e_bins), np.array(g_bins)
    return float(((g_bins - e_bins) ** 2 / e_bins).sum()), len(e_bins) - 1


def chi_square_sf(x, dof):
    """P(chi-square with dof degrees of freedom > x), by the finite series of the incomplete gamma function at half-integer and integer shape:
    even dof = 2 m: e^(-x/2) sum_{i < m} (x/2)^i / i!;  odd dof = 2 m + 1: erfc(sqrt(x/2)) + e^(-x/2) sum_{i < m} (x/2)^(i + 1/2) / Gamma(i + 3/2).
    Every term is positive and formed in logarithms"""
    h, m = 0.5 * x, dof // 2
    if x <= 0:
        return 1.0
    i = np.arange(m, dtype=np.float64)
    if dof % 2 == 0:
        logs = i * math.log(h) - np.array([math.lgamma(v + 1.0) for v in i]) - h
        return float(np.exp(logs).sum())
    logs = (i + 0.5) * math.log(h) - np.array([math.lgamma(v + 1.5) for v in i]) - h
    return math.erfc(math.sqrt(h)) + float(np.exp(logs).sum())


def chi_square_quantile(dof, tail=1e-6):
    """the 1 - tail quantile of the chi-square distribution with dof degrees of freedom: chi_square_sf solved by bisection to 1e-9 relative"""
    lo, hi = 0.0, float(dof) + 100.0 * math.sqrt(2.0 * dof) + 100.0
    assert chi_square_sf(hi, dof) < tail
    while hi - lo > 1e-9 * hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi_square_sf(mid, dof) > tail else (lo, mid)
    return hi


def counts_of(samples, chains):
    """int64[n]: how often each row of `chains` (unique rows, sorted as np.unique leaves them) occurs among `samples`; every sample must be one"""
    key = {c.tobytes(): i for i, c in enumerate(chains)}
    uniq, n = np.unique(np.asarray(samples, dtype=np.uint8), axis=0, return_counts=True)
    out = np.zeros(len(chains), dtype=np.int64)
    for c, k in zip(uniq, n):
        assert c.tobytes() in key, "a sample lies outside its class"
        out[key[c.tobytes()]] = k
    return out
