"""The L = 5 exact reference of the plaquette codes (util_exact.PlaquetteWeightEnumerator: 2^24 group elements per class, met in
the middle) against the L = 3 enumeration it generalises, and the oracle's random-scan (scan = 0) and shared-pick (scan = 3) chains
against it -- the CPU half of the first exact pin with 24 generators, length-5 logical operators and L = 5 boundary stencils (the GPU
half: tests/test_gpu_stats.py::test_plaquette_exact_L5)."""
import types

import numpy as np
import pytest

from oracle import oracle as orc
from util_exact import (PlaquetteWeightEnumerator, SurfEnumeration, alpha_counts_weight, biased_counts_weight, biased_weight,
                        depolarizing_counts_weight, depolarizing_weight)

ORC_API = types.SimpleNamespace(apply_stabilizer=orc.surf_apply_stabilizer, apply_logical=orc.surf_apply_logical,
                                eq_class=orc.surf_eq_class, ngen=orc.surf_ngen, gen_rco=orc.surf_gen_rco)


def _rand_surf(seed, L=3, p=0.3):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 4, size=(L, L)) * (rng.random((L, L)) < p)).astype(np.uint8)


_CACHE = {}


def _enum(code, init):
    key = (code, init.tobytes())
    if key not in _CACHE:                           # (about 1 s per syndrome at L = 5)
        _CACHE[key] = PlaquetteWeightEnumerator(code, init, ORC_API)
    return _CACHE[key]


@pytest.mark.parametrize("code", [orc.XZZX, orc.ROTATED])
@pytest.mark.parametrize("seed", [5, 6, 7])
def test_weight_enumerator_equals_the_full_enumeration_at_L3(code, seed):
    init = _rand_surf(seed)
    full, mitm = SurfEnumeration(code, init, ORC_API), PlaquetteWeightEnumerator(code, init, ORC_API)
    assert np.all(mitm.H.sum(axis=(1, 2)) == 2 ** mitm.G)
    for a, b in ((depolarizing_weight(0.2), depolarizing_counts_weight(0.2)), (depolarizing_weight(0.07), depolarizing_counts_weight(0.07)),
                 (biased_weight(0.25, 3.0), biased_counts_weight(0.25, 3.0, 9)), (biased_weight(0.15, 100.0), biased_counts_weight(0.15, 100.0, 9))):
        assert np.abs(full.class_probabilities(a) - mitm.class_probabilities(b)).max() < 1e-12
    # the alpha weight pz_tilde^(n_z + alpha (n_x + n_y)), written out on the full list of configurations
    pzt, alpha = 0.3, 2.5
    cfg = full.cfg
    direct = pzt ** ((cfg == 3).sum(-1) + alpha * ((cfg == 1) | (cfg == 2)).sum(-1))
    P = direct.sum(axis=1) / direct.sum()
    assert np.abs(P - mitm.class_probabilities(alpha_counts_weight(pzt, alpha))).max() < 1e-12


@pytest.mark.parametrize("code", [orc.XZZX, orc.ROTATED])
def test_weight_enumerator_at_L5_counts_every_group_element_once(code):
    init = _rand_surf(50 + code, 5, 0.2)
    e = _enum(code, init)
    assert e.G == 24
    assert np.all(e.H.sum(axis=(1, 2)) == 2 ** 24) and (e.H >= 0).all()
    P = e.class_probabilities(depolarizing_counts_weight(0.17))
    assert abs(P.sum() - 1) < 1e-12 and (P > 0).all()
    # representative independence: a stabilizer and a logical operator away, the same law (classes relabelled by the operator)
    m2 = orc.surf_apply_stabilizer(code, init, 2, 3, 1)[0]
    assert np.allclose(P, _enum(code, m2).class_probabilities(depolarizing_counts_weight(0.17)), rtol=1e-12)
    # the weights are read off the right axes: n_xy counts X and Y, n_z counts Z only (the counts of the seed's own class)
    c0 = int(orc.surf_eq_class(code, init))
    nxy, nz = int(((init == 1) | (init == 2)).sum()), int((init == 3).sum())
    assert e.H[c0, nxy, nz] >= 1


def _check_classes(frac, P, nsig=5.0, floor=3e-4, rare=0.75):
    """as tests/test_stats_cpu.py: 5 sigma on the classes that carry weight, a relative allowance on the rare ones"""
    mean, sem = frac.mean(axis=0), frac.std(axis=0, ddof=1) / np.sqrt(frac.shape[0])
    big = P >= 0.01
    assert np.all(np.abs(mean - P)[big] <= nsig * sem[big] + floor), (mean, P, sem)
    assert np.all(np.abs(mean - P)[~big] <= nsig * sem[~big] + rare * P[~big] + floor), (mean, P, sem)
    return mean, sem


L5_CASES = [(orc.XZZX, 65, 0.17, 5), (orc.ROTATED, 67, 0.17, 5)]


@pytest.mark.parametrize("scan", [0, 3])
@pytest.mark.parametrize("code,seed,p,Nc", L5_CASES)
def test_oracle_matches_exact_enumeration_L5(code, seed, p, Nc, scan):
    """The oracle's chains at L = 5 on the exact law.  scan = 3: every replica gets a pick group of its own (first_syndrome = 64 r),
    so the replicas are independent and their standard error means what it says."""
    init = _rand_surf(seed, 5, 0.2)
    P = _enum(code, init).class_probabilities(depolarizing_counts_weight(p))
    R, steps = 128, 4000
    if scan == 0:
        res = orc.pteq_batch(code, np.broadcast_to(init, (R,) + init.shape).copy(), p, Nc, steps, iters=10, tops_burn=5, seed=800 + seed,
                             n_threads=8)
        counts, samples = res["counts"], res["samples"]
    else:
        counts, samples = [], []
        for r in range(R):
            res = orc.pteq_batch(code, init[None].copy(), p, Nc, steps, iters=10, tops_burn=5, seed=800 + seed, first_syndrome=64 * r,
                                 n_threads=1, scan=3)
            counts.append(res["counts"][0]); samples.append(res["samples"][0])
        counts, samples = np.array(counts), np.array(samples)
    assert (samples > steps // 2).all()
    mean, _ = _check_classes(counts / samples[:, None].astype(np.float64), P)
    if np.sort(P)[-1] - np.sort(P)[-2] > 0.01:        # (some L = 5 syndromes tie classes exactly: xzzx seed 61 ties all four)
        assert mean.argmax() == P.argmax()
