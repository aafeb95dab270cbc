"""The CPU twin of qecmc.pteq_shortest_batch: the oracle's plain Ladder (alpha rule, scan = 3 "wave" or 2 "colour"), one per ladder, stepped on
Philox (seed, first_syndrome + l), with the bookkeeping of PTEQ_alpha_with_shortest (decoders_biasednoise.py:93-172) around it at two levels:

  (i)  raw(): the rule written out -- per class the smallest n_eff ATTRIBUTE of the bottom slot after burn-in, how often it was seen and the distinct
       configurations seen with it -- giving the arrays the kernels return, plus what the tests' preconditions look at;
  (ii) triple(): qecmc.decoders_biasednoise._shortest_loop (pinned to the reference by tests/golden f_nalpha.npz) on the same ladder, giving the three
       percent vectors.

The error_based criterion of level (i) is formed as the kernels and the oracle's PTEQ form it: exact integer window sums of (n_z, n_x + n_y), each mean
(sum n_z + alpha sum n_xy) / len.  Results are cached per argument tuple: the GPU tests of both scans and several properties share one computation."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import oracle as orc

SCAN = {"wave": 3, "colour": 2}
CODE = {"xzzx": orc.XZZX, "rotated": orc.ROTATED}
SENTINEL = 100000.0


def make_init(L, Nc, N):
    """the issue's inputs, drawn ladder by ladder: a ladder's Paulis, then its 12 % mask"""
    rng = np.random.default_rng(L * 5 + Nc + N)
    out = np.zeros((N, L, L), dtype=np.uint8)
    for l in range(N):
        paulis = rng.integers(1, 4, (L, L))
        out[l] = (paulis * (rng.random((L, L)) < 0.12)).astype(np.uint8)
    return out


class OracleLadder:
    """what _shortest_loop needs of a Ladder_alpha: .step(iters), .tops0, .chains[0].n_eff, .chains[0].code"""

    def __init__(self, code, init, pz_tilde, alpha, Nc, scan, rng):
        self._code, self._rng = code, rng
        self._ld = orc.Ladder(code, init, pz_tilde, Nc, p_logical=0.5, noise=orc.ALPHA, alpha=alpha, det_pow=1, scan=scan)
        self.chains = [self]
        self.code = SimpleNamespace(nbr_eq_classes=4, define_equivalence_class=self._cls, qubit_matrix=None)
        self._refresh()

    def _cls(self):
        return orc.surf_eq_class(self._code, self.code.qubit_matrix)

    def _refresh(self):
        self.code.qubit_matrix = self._ld.states[0]
        self.n_eff = float(self._ld.n_eff[0])
        self.counts = self._ld.n_eff_counts[0]          # (n_z, n_x + n_y) behind the attribute
        self.tops0 = self._ld.tops0

    def step(self, iters):
        self._ld.step(iters, self._rng)
        self._refresh()


def _one(code, init, pz_tilde, alpha, Nc, steps, iters, scan, crit, SEQ, TOPS, tops_burn, eps, seed, syndrome):
    ld = OracleLadder(code, init, pz_tilde, alpha, Nc, scan, orc.Rng.philox(seed, syndrome))
    counts = np.zeros(4, dtype=np.uint32)
    shortest, shortest_n = [SENTINEL] * 4, [0] * 4
    unique = [set() for _ in range(4)]
    offered, falls = set(), [0] * 4
    log = []                                             # (n_z, n_xy) per sample
    tops0 = samples = stale = 0
    conv_start = conv_streak = 0
    steps_done, converged = steps, False
    for step in range(steps):
        ld.step(iters)
        if ld.tops0 >= tops_burn:
            samples += 1
            m = ld.code.qubit_matrix
            c, v, cfg = int(ld._cls()), ld.n_eff, m.tobytes()
            counts[c] += 1
            log.append((int(ld.counts[0]), int(ld.counts[1])))
            own = float(np.count_nonzero(m == 3)) + alpha * float(np.count_nonzero((m == 1) | (m == 2)))
            stale += own != v
            if v < shortest[c]:
                shortest[c], shortest_n[c], unique[c] = v, 1, {cfg}
                falls[c] += 1
                offered.add((cfg, v))
            elif v == shortest[c]:
                shortest_n[c] += 1
                unique[c].add(cfg)
                offered.add((cfg, v))
        if crit and ld.tops0 >= TOPS:
            l = samples
            q2, q4 = log[l // 4: l // 2], log[3 * l // 4: l]
            accept = False
            if l and q2 and q4:
                m2 = (float(sum(z for z, _ in q2)) + alpha * float(sum(x for _, x in q2))) / float(len(q2))
                m4 = (float(sum(z for z, _ in q4)) + alpha * float(sum(x for _, x in q4))) / float(len(q4))
                accept = abs(m2 - m4) < eps
            if accept:
                if conv_streak >= SEQ:
                    steps_done, converged = step + 1, True
                    break
                conv_streak = ld.tops0 - conv_start
            else:
                conv_streak, conv_start = 0, ld.tops0
    tops0 = ld.tops0
    return dict(counts=counts, samples=samples, tops0=tops0, steps_done=steps_done, converged=converged, shortest=shortest, shortest_n=shortest_n,
                unique_n=[len(u) for u in unique], offered=len(offered), falls=max(falls), stale=int(stale))


@functools.lru_cache(maxsize=None)
def raw(code, L, Nc, N, steps, iters, pz_tilde, alpha, scan, crit=False, SEQ=2, TOPS=10, tops_burn=2, eps=0.1, seed=31, first=0, lo=0, hi=None):
    """level (i) on ladders lo .. hi of the issue's inputs for (L, Nc, N): the kernels' nine arrays (overflow is the caller's: offered > set_capacity), and
    per ladder `offered` (distinct (configuration, value) pairs offered to the set), `falls` (how often the minimum of its most active class fell, the first
    value included) and `stale` (samples whose attribute differs from the configuration's own n_z + alpha (n_x + n_y))"""
    init = make_init(L, Nc, N)
    hi = N if hi is None else hi
    rows = [_one(CODE[code], init[l], pz_tilde, alpha, Nc, steps, iters, SCAN[scan], crit, SEQ, TOPS, tops_burn, eps, seed, first + l) for l in range(lo, hi)]
    out = dict(counts=np.array([r["counts"] for r in rows], dtype=np.uint32), samples=np.array([r["samples"] for r in rows], dtype=np.uint32),
               tops0=np.array([r["tops0"] for r in rows], dtype=np.uint32), steps_done=np.array([r["steps_done"] for r in rows], dtype=np.uint32),
               converged=np.array([r["converged"] for r in rows], dtype=bool), shortest=np.array([r["shortest"] for r in rows], dtype=np.float64),
               shortest_n=np.array([r["shortest_n"] for r in rows], dtype=np.uint32), unique_n=np.array([r["unique_n"] for r in rows], dtype=np.uint32),
               offered=np.array([r["offered"] for r in rows]), falls=np.array([r["falls"] for r in rows]), stale=np.array([r["stale"] for r in rows]))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def triple(code, L, Nc, N, steps, iters, pz_tilde, alpha, scan, crit=False, SEQ=2, TOPS=10, tops_burn=2, eps=0.1, seed=31, first=0):
    """level (ii): _shortest_loop's three vectors per ladder -> (uint8[N,4], float64[N,4], float64[N,4])"""
    from qecmc.decoders_biasednoise import _shortest_loop
    init = make_init(L, Nc, N)
    rows = []
    for l in range(N):
        ld = OracleLadder(CODE[code], init[l], pz_tilde, alpha, Nc, SCAN[scan], orc.Rng.philox(seed, first + l))
        rows.append(_shortest_loop(ld, pz_tilde, SEQ, TOPS, tops_burn, eps, steps, iters, 'error_based' if crit else None))
    out = tuple(np.array([r[k] for r in rows]) for k in range(3))
    for v in out:
        v.setflags(write=False)
    return out
