"""The equilibrium observables of qecmc_plan_set_stats / pteq_batch(return_swap_stats=True) from the scan = "wave" and scan = "colour" kernels
(csrc/ladder_wu.hpp STATS, csrc/ladder_colour.hpp: ladder_wu_stats_kernel, ladder_colour_stats_kernel): per ladder, the steps in which each rung pair
traded states (the untested trades of ne_hi <= ne_lo included; the alpha rule: the n_eff test) and the sum over the steps of every slot's error count
after the step's swaps -- Ladder.r_flip's outcomes and count_errors per rung, src/mcmc.py:85-103.

  * bit for bit against the CPU oracle's ladder under the same scan (oracle.Ladder(..., scan=3 | 2), which keeps both counters for all three rules);
  * the counters do not disturb the run: counts, samples, tops0 and the final states equal those of the same call without statistics, which runs the
    fast kernel -- the two instantiations of the one program;
  * what stays refused: the criterion on either layout, the 32-word wave shapes, replicas > 1;
  * fixture F5 (the reference's own 20 000-step ladders) on the wave kernel with its own counters, under the allowances of the random-scan branch of
    tests/test_gpu_round2.py::test_reference_equilibrium_observables_f5: a single ladder has the same law under both scans (the pick never depends on
    the state), so the per-replica window averages are distributed as there; the correlation between the 64 ladders of a wavefront is what the
    standard error over the wavefront means accounts for."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

N, FIRST, STEPS, SEED = 70, 64, 120, 5
LADDERS = (0, 1, 33, 63, 64, 69)          # both ends of the first wavefront / workgroup, the second one's first and last live lane

# (id, scan, code, L, Nc, p, iters, rule): rule = {} (depolarizing), {"eta": ..} (biased), {"alpha": ..} (alpha; p is then pz_tilde)
CASES = [
    ("wave-toric-L3-Nc2", "wave", "toric", 3, 2, 0.1, 10, {}),                       # the 4-word kernel
    ("wave-toric-L5-Nc5", "wave", "toric", 5, 5, 0.1, 10, {}),
    ("wave-toric-L9-Nc8", "wave", "toric", 9, 8, 0.15, 10, {}),                      # 12 words: the headline shape
    ("wave-toric-L11-Nc3", "wave", "toric", 11, 3, 0.12, 10, {}),                    # 16 words
    ("wave-toric-L5-Nc12", "wave", "toric", 5, 12, 0.1, 10, {}),                     # more than 8 rungs
    ("wave-rotated-L7-Nc7", "wave", "rotated", 7, 7, 0.17, 7, {}),
    ("wave-xzzx-L5-Nc4", "wave", "xzzx", 5, 4, 0.15, 1, {}),
    ("wave-planar-L5-Nc5", "wave", "planar", 5, 5, 0.12, 10, {}),
    ("wave-alpha-xzzx-L5-Nc5", "wave", "xzzx", 5, 5, 0.175, 10, {"alpha": 4.04}),
    ("wave-alpha-rotated-L5-Nc4", "wave", "rotated", 5, 4, 0.15, 10, {"alpha": 3.0}),
    ("colour-toric-L5-Nc5", "colour", "toric", 5, 5, 0.1, 10, {}),
    ("colour-rotated-L7-Nc7", "colour", "rotated", 7, 7, 0.17, 10, {}),
    ("colour-planar-L5-Nc5", "colour", "planar", 5, 5, 0.12, 10, {}),
    ("colour-biased-xzzx-L5-Nc4", "colour", "xzzx", 5, 4, 0.15, 10, {"eta": 100.0}),
    ("colour-alpha-xzzx-L5-Nc5", "colour", "xzzx", 5, 5, 0.175, 10, {"alpha": 4.04}),
]


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _init(name, L, Nc, p):
    rng = np.random.default_rng(L * 10 + Nc)
    m = np.zeros((N, 2, L, L) if name in ("toric", "planar") else (N, L, L), dtype=np.uint8)
    err = rng.random(m.shape) < p
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    if name == "planar":
        m[:, 1, -1, :] = 0; m[:, 1, :, -1] = 0
    return m


_RUNS = {}


def _run(q, case):
    """one case on the GPU, once for the module: the call with statistics and the same call without them"""
    cid, scan, name, L, Nc, p, iters, rule = case
    if cid not in _RUNS:
        init = _init(name, L, Nc, 0.12 if "alpha" in rule else p)
        code = {"toric": q.TORIC, "xzzx": q.XZZX, "rotated": q.ROTATED, "planar": q.PLANAR}[name]
        kw = dict(Nc=Nc, steps=STEPS, iters=iters, tops_burn=0, seed=SEED, first_syndrome=FIRST, code=code, scan=scan, return_states=True, **rule)
        _RUNS[cid] = (init, q.pteq_batch(init, p, return_swap_stats=True, **kw), q.pteq_batch(init, p, **kw))
    return _RUNS[cid]


def _oracle_stats(orc, case, init, syn):
    """tests/test_gpu_round2.py _oracle_stats with the scan and the rule passed through"""
    _, scan, name, L, Nc, p, iters, rule = case
    code = {"toric": orc.TORIC, "xzzx": orc.XZZX, "rotated": orc.ROTATED, "planar": orc.PLANAR}[name]
    noise = orc.ALPHA if "alpha" in rule else orc.BIASED if "eta" in rule else orc.DEPOLARIZING
    ld = orc.Ladder(code, init, p, Nc, 0.5, noise=noise, eta=rule.get("eta", 0.0), alpha=rule.get("alpha", 0.0), det_pow=1 if "alpha" in rule else 0,
                    scan=3 if scan == "wave" else 2)
    rng = orc.Rng.philox(SEED, syn)
    for _ in range(STEPS):
        ld.step(iters, rng)
    return ld.swap_accepts, ld.nerr_sums


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_swap_and_error_statistics_bit_exact(q, orc, case):
    Nc = case[4]
    init, got, _ = _run(q, case)
    assert got["swap_accepts"].shape == (N, Nc - 1) and got["nerr_sums"].shape == (N, Nc)
    for s in LADDERS:
        acc, nsum = _oracle_stats(orc, case, init[s], FIRST + s)
        assert np.array_equal(got["swap_accepts"][s], acc.astype(np.uint32)), (s, got["swap_accepts"][s], acc)
        assert np.array_equal(got["nerr_sums"][s], nsum.astype(np.uint32)), (s, got["nerr_sums"][s], nsum)
    # (the two-rung L = 3 ladders never trade in 120 steps -- the oracle's neither: their top rung sits a dozen errors above the bottom one)
    assert (got["swap_accepts"].any() or Nc == 2) and (got["swap_accepts"] <= STEPS).all() and got["nerr_sums"].any()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_counters_do_not_disturb_the_run(q, case):
    _, got, plain = _run(q, case)
    for k in ("counts", "samples", "tops0", "states"):
        assert np.array_equal(got[k], plain[k]), k
    assert got["counts"].sum() > 0


@pytest.mark.parametrize("scan", ["wave", "colour"])
def test_statistics_with_the_criterion_stay_refused(q, scan):
    init = _init("toric", 5, 5, 0.1)
    with pytest.raises(q.QecmcError, match="not with the criterion"):
        q.pteq_batch(init, 0.1, Nc=5, steps=200, scan=scan, conv_criteria="error_based", return_swap_stats=True)


def test_statistics_of_the_32_word_wave_shapes_stay_refused(q):
    init = _init("toric", 15, 4, 0.1)[:64]
    with pytest.raises(q.QecmcError, match="above 16 state words"):
        q.pteq_batch(init, 0.1, Nc=4, steps=10, scan="wave", return_swap_stats=True)
    assert q.pteq_batch(init, 0.1, Nc=4, steps=10, scan="wave")["samples"].shape == (64,)      # (the shape itself runs)


@pytest.mark.parametrize("scan", ["wave", "colour"])
def test_statistics_with_replicas_stay_refused(q, scan):
    init = _init("toric", 5, 5, 0.1)[:4]
    with pytest.raises(q.QecmcError, match="replicas"):
        q.pteq_batch(init, 0.1, Nc=5, steps=20, scan=scan, replicas=2, return_swap_stats=True)


def _wavefront_se(x):
    """standard error of the mean of x[R, ...] over its 64-ladder groups (scan = "wave": the ladders of a wavefront share their picks)"""
    g = x.reshape(-1, 64, *x.shape[1:]).mean(axis=1)
    return g.std(axis=0, ddof=1) / np.sqrt(g.shape[0])


@pytest.mark.parametrize("name", ["toric_L9", "rot_L5", "rot_L7"])
def test_reference_equilibrium_observables_f5_wave_counters(q, name):
    """Fixture F5 on the wave kernel with its own counters.  Settings of the random-scan branch of tests/test_gpu_round2.py
    test_reference_equilibrium_observables_f5: the window is the run of `steps` minus the run of `burn` (an exact prefix), 4 096 replicas per syndrome,
    the GPU's standard error over the 64 wavefront means.  Allowances of that branch, unchanged: swap acceptance 1e-3 on the medians and 5e-3 on the
    means, per-rung <n> 0.02 and 5e-3 max, 4.5 combined standard errors."""
    g = np.load(os.path.join(GOLDEN, "f5_stats.npz"))
    L, p, eta, Nc, iters, steps, burn = g[f"{name}_par"]
    L, Nc, iters, steps, burn = int(L), int(Nc), int(iters), int(steps), int(burn)
    code = q.TORIC if name.startswith("toric") else q.ROTATED
    kw = dict(Nc=Nc, iters=iters, tops_burn=0, code=code, scan="wave", return_swap_stats=True)
    R, win = 4096, steps - burn
    for s in range(g[f"{name}_init"].shape[0]):
        init = np.broadcast_to(g[f"{name}_init"][s], (R,) + g[f"{name}_init"][s].shape).copy()
        a = q.pteq_batch(init, float(p), steps=burn, seed=600 + s, **kw)
        b = q.pteq_batch(init, float(p), steps=steps, seed=600 + s, **kw)
        r_acc = g[f"{name}_swap_acc"][s] / g[f"{name}_swap_att"][s]
        r_n = g[f"{name}_nerr"][s]

        def close(what, ref, gpu, floor, loose):
            se = np.sqrt(ref.var(axis=0, ddof=1) / ref.shape[0] + _wavefront_se(gpu) ** 2)
            dm = np.abs(np.median(ref, axis=0) - np.median(gpu, axis=0))
            d = np.abs(ref.mean(axis=0) - gpu.mean(axis=0))
            print(name, s, what, "medians: worst excess over 4.5 * 1.2533 se", float((dm - 4.5 * 1.2533 * se).max()), "allowed", floor,
                  "| means: worst excess over 4.5 se", float((d - 4.5 * se).max()), "allowed", loose)
            assert np.all(dm <= 4.5 * 1.2533 * se + floor), (name, s, what, "medians", np.median(ref, axis=0), np.median(gpu, axis=0), se)
            assert np.all(d <= 4.5 * se + loose), (name, s, what, "means", ref.mean(axis=0), gpu.mean(axis=0), se)
        acc = (b["swap_accepts"].astype(np.int64) - a["swap_accepts"]) / win          # [R, Nc-1] acceptance per replica
        nerr = (b["nerr_sums"].astype(np.int64) - a["nerr_sums"]) / win               # [R, Nc]
        close("swap acceptance", r_acc, acc, 1e-3, 5e-3)
        close("per-rung <n>", r_n, nerr, 0.02, 5e-3 * r_n.mean(axis=0).max())
