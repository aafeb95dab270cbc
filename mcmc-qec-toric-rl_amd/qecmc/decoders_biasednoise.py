"""Host-side mirror of `PTEQ_biased` (decoders_biasednoise.py:28-75) and `PTEQ_alpha` (:175-226): the PTEQ loop around
Ladder_biased / Ladder_alpha; `PTEQ_alpha_with_shortest` (:93-172) as that loop on the host or, batched, in the kernels."""
import numpy as np

from . import _lib as L_
from .decoders import _pteq
from .mcmc import _code_id, _fresh_seed


def PTEQ_biased(init_code, p, eta=0.5, Nc=None, SEQ=2, TOPS=10, tops_burn=2, eps=0.1, steps=50000000, iters=10,
                conv_criteria='error_based', seed=None, replicas=None, scan="random"):
    """decoders_biasednoise.PTEQ_biased (:28-90).  scan="colour": the one-syndrome latency layout (a workgroup per ladder, a colour phase of
    generators per wavefront pass; every generator a Metropolis move for the biased weight -- the reference's rule at iters = 1)."""
    return _pteq(init_code, p, eta, Nc, SEQ, TOPS, tops_burn, eps, steps, iters, conv_criteria, seed, replicas=replicas, scan=scan)


def PTEQ_alpha(init_code, pz_tilde, alpha=1, Nc=None, SEQ=2, TOPS=10, tops_burn=2, eps=0.1, steps=50000000, iters=10,
               conv_criteria='error_based', seed=None, replicas=None, scan="random"):
    """decoders_biasednoise.PTEQ_alpha (:175-238).  scan="colour": the one-syndrome latency layout; scan="wave": the batched throughput layout."""
    return _pteq(init_code, pz_tilde, None, Nc, SEQ, TOPS, tops_burn, eps, steps, iters, conv_criteria, seed, alpha=alpha, replicas=replicas, scan=scan)


def _shortest_loop(ladder, pz_tilde, SEQ, TOPS, tops_burn, eps, steps, iters, conv_criteria):
    """The bookkeeping of PTEQ_alpha_with_shortest (decoders_biasednoise.py:93-172) around any Ladder_alpha-like object
    (`.step(iters)`, `.tops0`, `.chains[0].n_eff`, `.chains[0].code`).  Besides PTEQ_alpha's class histogram it keeps, per
    class, the smallest n_eff the bottom slot showed after burn-in, how often, and the distinct configurations seen with it."""
    import warnings
    import numpy as np
    from math import exp
    nbr_eq_classes = ladder.chains[0].code.nbr_eq_classes
    counts = np.zeros(nbr_eq_classes, dtype=np.uint32)                 # eq[since_burn], kept as a running row (:103,:123-124)
    log = np.zeros(1024)                                               # nbr_errors_bottom_chain, grown on demand (:101)
    since_burn = burn = 0
    conv_start = conv_streak = 0
    unique = [dict() for _ in range(nbr_eq_classes)]                   # :112
    shortest_n = [0] * nbr_eq_classes
    shortest = [100000] * nbr_eq_classes
    for step in range(int(steps)):
        ladder.step(iters)                                             # :120
        bottom = ladder.chains[0]
        cls = int(bottom.code.define_equivalence_class())              # :122
        if ladder.tops0 >= tops_burn:                                  # :124
            since_burn = step - burn
            counts[cls] += 1
            if since_burn >= log.size:
                log = np.concatenate([log, np.zeros(log.size)])
            n_eff = log[since_burn] = bottom.n_eff                     # :128 -- the slot's attribute, possibly stale (quirk Q4)
            if n_eff < shortest[cls]:                                  # :130-138: a new minimum restarts the class's set
                shortest_n[cls], shortest[cls] = 1, n_eff
                unique[cls] = {bottom.code.qubit_matrix.tobytes(): n_eff}
            elif n_eff == shortest[cls]:                               # :139-144
                shortest_n[cls] += 1
                unique[cls].setdefault(bottom.code.qubit_matrix.tobytes(), n_eff)
        else:
            burn += 1                                                  # :147
        if conv_criteria == 'error_based' and ladder.tops0 >= TOPS:    # :149-157; the criterion of :226-238
            l = since_burn + 1
            with np.errstate(invalid="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")                       # an empty quarter averages to nan: not accepted
                err = abs(np.average(log[l // 4: l // 2]) - np.average(log[3 * l // 4: l]))
            if err < eps:
                if conv_streak >= SEQ:
                    break
                conv_streak = ladder.tops0 - conv_start
            else:
                conv_streak, conv_start = 0, ladder.tops0
    beta = -np.log(pz_tilde)                                           # :163
    eqdistr = np.array([sum(exp(-beta * v) for v in u.values()) for u in unique])       # :165-167
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((np.divide(counts, since_burn + 1) * 100).astype(np.uint8), np.divide(eqdistr, sum(eqdistr)) * 100,
                np.array(shortest_n) / sum(shortest_n) * 100)          # :170


def pteq_shortest_batch(init, pz_tilde, alpha, Nc=None, steps=1000, iters=10, tops_burn=2, p_logical=0.5, seed=0, first_syndrome=0, device=0,
                        conv_criteria=None, SEQ=2, TOPS=10, eps=0.1, code=L_.XZZX, scan="wave", set_capacity=1024, return_stats=False, flags=0,
                        replicas=1, return_swap_stats=False):
    """PTEQ_alpha_with_shortest (decoders_biasednoise.py:93-172) on N syndromes at once, bookkeeping in the kernels.

    init: uint8[N, L, L] seed configurations of the xzzx / rotated code; scan="wave" (the batched throughput layout; first_syndrome a multiple of 64)
    or scan="colour" (a workgroup per ladder).  Every ladder keeps one lane (one workgroup) for the whole run, so its results depend on (seed, first_syndrome
    + index) alone.  conv_criteria None runs exactly `steps` ladder steps, 'error_based' stops each ladder by the reference's criterion.
    Besides pteq_batch's counts uint32[N,4], samples, tops0, steps_done uint32[N] and converged bool[N], per ladder and class: shortest float64[N,4] (the
    smallest n_eff attribute the bottom slot showed after burn-in; 100000.0, the reference's sentinel, for a class never seen), shortest_n uint32[N,4] (the
    samples with it), unique_n uint32[N,4] (the distinct configurations among them) and overflow bool[N]: the ladder offered more than `set_capacity`
    distinct (configuration, value) pairs to its set, and its unique_n row is unspecified.  shortest_distribution() turns them into the reference's vectors.
    The statistics are per ladder and come from kernels of their own: replicas > 1 and return_swap_stats=True (pteq_batch's counters) are refused."""
    if return_swap_stats:
        raise L_.QecmcError("qecmc_plan_set_shortest: not together with qecmc_plan_set_stats (the shortest-chain kernels carry no swap counters)")
    if conv_criteria not in (None, 'error_based'):
        raise ValueError(f"conv_criteria={conv_criteria!r}: only None and 'error_based' exist for PTEQ")
    if scan not in L_.SCANS:
        raise ValueError(f"scan={scan!r}")
    a, _ = L_.as_states(init, 3 if code in (L_.TORIC, L_.PLANAR) else 2)
    N, size = a.shape[0], a.shape[-1]
    Nc = Nc or size
    pr = L_.make_params(code=code, L=size, Nc=Nc, p=float(pz_tilde), p_logical=float(p_logical), iters=int(iters), steps=int(steps),
                        tops_burn=int(tops_burn), TOPS=int(TOPS), SEQ=int(SEQ), eps=float(eps), seed=seed, first_syndrome=first_syndrome, device=device,
                        conv_mode=L_.CONV_ERROR_BASED if conv_criteria else L_.CONV_NONE, noise=L_.NOISE_DEPOLARIZING if alpha is None else L_.NOISE_ALPHA,
                        alpha=0.0 if alpha is None else float(alpha), scan=L_.SCANS[scan], flags=int(flags), replicas=int(replicas))
    ncls = 16 if code == L_.TORIC else 4
    counts = np.zeros((N, ncls), dtype=np.uint32)
    samples, tops0, steps_done = (np.zeros(N, dtype=np.uint32) for _ in range(3))
    converged, overflow = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
    shortest = np.full((N, 4), 100000.0, dtype=np.float64)
    shortest_n, unique_n = np.zeros((N, 4), dtype=np.uint32), np.zeros((N, 4), dtype=np.uint32)
    stats = L_.Stats()
    import ctypes as C
    L_.check(L_.lib().qecmc_pteq_batch_shortest(pr, L_.u8(a), N, int(set_capacity), L_.u32(counts), L_.u32(samples), L_.u32(tops0), L_.u32(steps_done),
                                                L_.u8(converged), shortest.ctypes.data_as(C.POINTER(C.c_double)), L_.u32(shortest_n), L_.u32(unique_n),
                                                L_.u8(overflow), stats))
    out = dict(counts=counts, samples=samples, tops0=tops0, steps_done=steps_done, converged=converged.astype(bool), shortest=shortest,
               shortest_n=shortest_n, unique_n=unique_n, overflow=overflow.astype(bool))
    if return_stats:
        out["stats"] = dict(proposals=int(stats.proposals), swap_tests=int(stats.swap_tests), kernel_ms=float(stats.kernel_ms), total_ms=float(stats.total_ms))
    return out


def shortest_distribution(res, pz_tilde):
    """The three percent vectors PTEQ_alpha_with_shortest returns (decoders_biasednoise.py:163-170), per ladder, from pteq_shortest_batch's arrays (a pure
    host function): (uint8[N,4] class counts / samples x 100, truncated; float64[N,4] eqdistr / sum x 100 with eqdistr[c] = unique_n[c] exp(-beta shortest[c]),
    beta = -ln(pz_tilde) -- every value the reference's dict holds equals the class's minimum --; float64[N,4] shortest_n / sum x 100).  The normalisation
    is the reference's: a ladder that never left burn-in divides by zero there and gives NaN rows here (the first vector: counts / 1, all zero); an
    overflowed ladder's second vector is NaN."""
    counts, samples = np.asarray(res["counts"]), np.asarray(res["samples"], dtype=np.float64)
    shortest, shortest_n = np.asarray(res["shortest"], dtype=np.float64), np.asarray(res["shortest_n"], dtype=np.float64)
    unique_n = np.asarray(res["unique_n"], dtype=np.float64)
    beta = -np.log(pz_tilde)
    with np.errstate(divide="ignore", invalid="ignore"):
        first = (np.divide(counts, np.maximum(samples, 1.0)[:, None]) * 100).astype(np.uint8)          # :170, since_burn + 1 = samples (1 before any)
        eq = np.where(unique_n > 0, unique_n * np.exp(-beta * shortest), 0.0)                           # :165-167 (an empty dict sums to 0)
        second = np.divide(eq, eq.sum(axis=1, keepdims=True)) * 100
        third = shortest_n / shortest_n.sum(axis=1, keepdims=True) * 100
    second[np.asarray(res["overflow"], dtype=bool)] = np.nan
    return first, second, third


def PTEQ_alpha_with_shortest(init_code, pz_tilde, alpha=1, Nc=None, SEQ=2, TOPS=10, tops_burn=2, eps=0.1, steps=50000000, iters=10,
                             conv_criteria='error_based', seed=None, scan="random", set_capacity=1024):
    """Drop-in for decoders_biasednoise.PTEQ_alpha_with_shortest (:93-172; generate_data.py:162-167, method
    "PTEQ_with_shortest"): returns (PTEQ_alpha's uint8 percent vector, the percent vector from the distinct shortest chains,
    the percent of observations at the shortest n_eff per class).  scan="random" (the default) is the reference's own chain: the ladder
    runs on the GPU one `Ladder_alpha.step` per launch and the bookkeeping on the host, so it is launch-bound (~10^4 ladder
    steps/s).  scan="colour" / "wave" run the one syndrome through pteq_shortest_batch: the whole run, bookkeeping included, is one
    launch (with the criterion, `steps` sizes its log: 4 B per step)."""
    if scan != "random":
        res = pteq_shortest_batch(init_code.qubit_matrix, pz_tilde, alpha, Nc=Nc or init_code.system_size, steps=steps, iters=iters, tops_burn=tops_burn,
                                  seed=_fresh_seed() if seed is None else seed, conv_criteria=conv_criteria, SEQ=SEQ, TOPS=TOPS, eps=eps,
                                  code=_code_id(init_code), scan=scan, set_capacity=set_capacity)
        first, second, third = shortest_distribution(res, pz_tilde)
        return first[0], second[0], third[0]
    from .mcmc_alpha import Ladder_alpha
    ladder = Ladder_alpha(pz_tilde, init_code, alpha, Nc or init_code.system_size, 0.5, seed=seed)     # :109
    return _shortest_loop(ladder, pz_tilde, SEQ, TOPS, tops_burn, eps, steps, iters, conv_criteria)


# decoders_biasednoise.py:79-90 / :226-237: the same criterion under two more names
from .decoders import conv_crit_error_based_PT as conv_crit_error_based_PT_biased     # noqa: E402
from .decoders import conv_crit_error_based_PT as conv_crit_error_based_PT_alpha      # noqa: E402
