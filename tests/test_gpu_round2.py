"""Round-2 additions of the HIP path against the pinned oracle: replica ladders (the small-batch mode), the equilibrium
observables (per-pair swap acceptances, per-rung error-count sums), exact chunked continuation, and the harness's shard /
resume / threshold-curve drivers.  Bit-exact wherever the oracle computes the same thing; fixture F5 (the reference's own
20 000-step runs at toric L=9, rotated L=5/7, biased xzzx L=5/7) closes the statistical loop where the benchmark lives."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def rand_states(rng, n, L, p):
    m = np.zeros((n, 2, L, L), dtype=np.uint8)
    err = rng.random(m.shape) < p
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    return m


def rand_plaq(rng, n, L, p):
    m = np.zeros((n, L, L), dtype=np.uint8)
    err = rng.random(m.shape) < p
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    return m


# ------------------------------------------------------------------ replicas
@pytest.mark.parametrize("N,R,L,Nc,first", [(5, 7, 5, 5, 0), (3, 64, 5, 4, 1000), (1, 100, 3, 3, 0), (70, 3, 5, 5, 17)])
def test_replicas_equal_R_separate_oracle_runs_summed(q, orc, N, R, L, Nc, first):
    rng = np.random.default_rng(N * 100 + R)
    init = rand_states(rng, N, L, 0.12)
    got = q.pteq_batch(init, 0.12, Nc=Nc, steps=150, iters=10, tops_burn=1, seed=99, first_syndrome=first, replicas=R, return_states=True)
    # ladder l = s*R + r starts from init[s] and draws from Philox syndrome index first + l
    ref = orc.toric_pteq_batch(np.repeat(init, R, axis=0), 0.12, Nc, 150, iters=10, tops_burn=1, seed=99, first_syndrome=first,
                               return_states=True)
    assert np.array_equal(got["counts"], ref["counts"].reshape(N, R, 16).sum(axis=1))
    assert np.array_equal(got["samples"], ref["samples"].reshape(N, R).sum(axis=1).astype(np.uint32))
    assert np.array_equal(got["tops0"], ref["tops0"].reshape(N, R).sum(axis=1).astype(np.uint32))
    assert np.array_equal(got["states"], ref["states"])                       # [N*R, Nc, ...] per ladder


def test_replicas_with_convergence_criterion(q, orc):
    rng = np.random.default_rng(8)
    init = rand_states(rng, 2, 3, 0.1)
    R = 20
    got = q.pteq_batch(init, 0.1, Nc=3, steps=4000, tops_burn=2, seed=4, replicas=R, conv_criteria="error_based", TOPS=6, SEQ=2, eps=0.2)
    ref = orc.toric_pteq_batch(np.repeat(init, R, axis=0), 0.1, 3, 4000, tops_burn=2, seed=4, conv_criteria="error_based", TOPS=6, SEQ=2, eps=0.2)
    assert ref["converged"].any()
    assert np.array_equal(got["counts"], ref["counts"].reshape(2, R, 16).sum(axis=1))
    assert np.array_equal(got["steps_done"], ref["steps_done"].reshape(2, R).max(axis=1).astype(np.uint32))   # the slowest ladder
    assert np.array_equal(got["converged"], ref["converged"].reshape(2, R).all(axis=1))


def test_pteq_dropin_replicas_are_opt_in(q, orc):
    """decoders.PTEQ(code, p) is one syndrome per call (decoders.py:25).  The drop-in's default is the reference's estimator, ONE
    ladder; replicas=64 (per call, or decoders.PTEQ_REPLICAS for a script) fills the wavefronts with independent ladders and
    forms the percent vector from their summed counts."""
    from qecmc import decoders
    assert decoders.PTEQ_REPLICAS == 1
    rng = np.random.default_rng(2)
    code = q.Toric_code(5)
    code.qubit_matrix = rand_states(rng, 1, 5, 0.1)[0]
    for R, kw in ((1, {}), (64, dict(replicas=64))):
        pct = q.PTEQ(code, 0.1, Nc=5, steps=300, iters=10, tops_burn=1, conv_criteria=None, seed=31, **kw)
        ref = orc.toric_pteq_batch(np.repeat(code.qubit_matrix[None], R, axis=0), 0.1, 5, 300, iters=10, tops_burn=1, seed=31)
        assert np.array_equal(pct, decoders.percent_from_counts(ref["counts"].sum(axis=0), ref["samples"].sum()))


# ------------------------------------------------------------------ swap / error-count observables
def _oracle_stats(orc, kind, init, p, Nc, steps, iters, seed, syn, eta=0.0):
    rng = orc.Rng.philox(seed, syn)
    if kind == "toric":
        ld = orc.ToricLadder(init, p, Nc, 0.5)
    else:
        code = {"xzzx": orc.XZZX, "xzzxb": orc.XZZX, "rot": orc.ROTATED, "planar": orc.PLANAR}[kind]
        ld = orc.Ladder(code, init, p, Nc, 0.5, noise=orc.BIASED if kind == "xzzxb" else orc.DEPOLARIZING, eta=eta)
    for _ in range(steps):
        ld.step(iters, rng)
    return ld.swap_accepts, ld.nerr_sums


@pytest.mark.parametrize("kind,L,Nc,p,eta", [("toric", 5, 5, 0.1, 0), ("toric", 9, 8, 0.15, 0), ("toric", 4, 2, 0.1, 0), ("rot", 7, 7, 0.17, 0),
                                             ("xzzx", 5, 4, 0.15, 0), ("xzzxb", 5, 5, 0.15, 100.0), ("planar", 5, 5, 0.12, 0)])
def test_swap_and_error_statistics_bit_exact(q, orc, kind, L, Nc, p, eta):
    rng = np.random.default_rng(L * 10 + Nc)
    N, steps = 70, 120
    if kind == "toric":
        init, code = rand_states(rng, N, L, p), q.TORIC
    elif kind == "planar":
        init, code = rand_states(rng, N, L, p), q.PLANAR
        init[:, 1, -1, :] = 0; init[:, 1, :, -1] = 0
    else:
        init, code = rand_plaq(rng, N, L, p), (q.ROTATED if kind == "rot" else q.XZZX)
    got = q.pteq_batch(init, p, Nc=Nc, steps=steps, iters=10, tops_burn=0, seed=5, first_syndrome=40, code=code,
                       eta=eta if kind == "xzzxb" else None, return_swap_stats=True)
    assert got["swap_accepts"].shape == (N, Nc - 1) and got["nerr_sums"].shape == (N, Nc)
    for s in (0, 1, 33, 63, 64, 69):
        acc, nsum = _oracle_stats(orc, kind, init[s], p, Nc, steps, 10, 5, 40 + s, eta)
        assert np.array_equal(got["swap_accepts"][s], acc.astype(np.uint32)), (s, got["swap_accepts"][s], acc)
        assert np.array_equal(got["nerr_sums"][s], nsum.astype(np.uint32)), (s, got["nerr_sums"][s], nsum)
    # the observables do not disturb the run
    plain = q.pteq_batch(init, p, Nc=Nc, steps=steps, iters=10, tops_burn=0, seed=5, first_syndrome=40, code=code,
                         eta=eta if kind == "xzzxb" else None)
    assert np.array_equal(plain["counts"], got["counts"]) and np.array_equal(plain["tops0"], got["tops0"])


F5_NAMES = ["toric_L9", "rot_L5", "rot_L7", "xzzxb_L5", "xzzxb_L7"]


def _wavefront_se(x):
    """standard error of the mean of x[R, ...] over its 64-ladder groups (scan = "wave": the ladders of a wavefront share their picks)"""
    g = x.reshape(-1, 64, *x.shape[1:]).mean(axis=1)
    return g.std(axis=0, ddof=1) / np.sqrt(g.shape[0])


@pytest.mark.parametrize("scan,name", [("random", n) for n in F5_NAMES] + [("wave", n) for n in ("toric_L9", "rot_L5", "rot_L7")])
def test_reference_equilibrium_observables_f5(q, name, scan):
    """Fixture F5: the reference's own ladders (R=16 replicas x 3 syndromes, 20 000 steps, first 20 % discarded) against the GPU
    (512 replicas per syndrome, the same run length and burn-in: a run of `burn` steps is the exact prefix of the run of
    `steps`, so the difference of the two is the post-burn-in window).  Per-rung <n_errors> and per-pair swap acceptance
    within the combined standard error; class histograms with the heavy-tail allowance of test_reference_histograms_f3.

    scan = "wave" (the benchmark's kernel; the biased ladders have no wave kernel) keeps no swap or per-rung counters, so: 4 096 replicas,
    the class histogram from the prefix difference as above, per-rung <n> from the final-state ensemble (one snapshot per replica:
    an equilibrium sample like the reference's window average, but not distributed like it, so only the means are compared -- the
    median of integer snapshots is not the median of 16 000-step averages), swap acceptance not at all (it is a property of the
    swap test, which the two scans share; random-scan only).  The GPU's standard error is taken over the 64 wavefront means.
    Runtime on the wave kernel: about 2 x 4096 x 20 000 x 8 rungs x 10 = 1.3e10 proposals per toric syndrome, a second or so."""
    from qecmc import toric_model as tm
    g = np.load(os.path.join(GOLDEN, "f5_stats.npz"))
    L, p, eta, Nc, iters, steps, burn = g[f"{name}_par"]
    L, Nc, iters, steps, burn = int(L), int(Nc), int(iters), int(steps), int(burn)
    code = q.TORIC if name.startswith("toric") else q.XZZX if name.startswith("xzzx") else q.ROTATED
    wave = scan == "wave"
    kw = dict(Nc=Nc, iters=iters, tops_burn=0, code=code, eta=float(eta) if name.startswith("xzzxb") else None, scan=scan)
    kw.update(return_states=True) if wave else kw.update(return_swap_stats=True)
    R, win = 4096 if wave else 512, steps - burn
    for s in range(g[f"{name}_init"].shape[0]):
        init = np.broadcast_to(g[f"{name}_init"][s], (R,) + g[f"{name}_init"][s].shape).copy()
        a = q.pteq_batch(init, float(p), steps=burn, seed=600 + s, **dict(kw, return_states=False))
        b = q.pteq_batch(init, float(p), steps=steps, seed=600 + s, **kw)
        hist = (b["counts"].astype(np.int64) - a["counts"]) / win
        r_acc = g[f"{name}_swap_acc"][s] / g[f"{name}_swap_att"][s]
        r_n = g[f"{name}_nerr"][s]
        r_h = g[f"{name}_hist"][s] / win

        def close(ref, gpu, floor, loose, medians=True):
            # Replicas that spend the window in another equivalence class sit in another mode of these observables (a run of
            # 16 000 steps does not always mix between classes: SURVEY 8d), so the reference's 16 replicas can miss a mode that
            # 1 in 10 of the GPU's 512 visits and their sample variance then understates the error of their mean.  Strict:
            # the medians (blind to a minority mode) within the combined standard error; loose: the means.
            gse = _wavefront_se(gpu) if wave else np.sqrt(gpu.var(axis=0, ddof=1) / gpu.shape[0])
            se = np.sqrt(ref.var(axis=0, ddof=1) / ref.shape[0] + gse ** 2)
            if medians:
                dm = np.abs(np.median(ref, axis=0) - np.median(gpu, axis=0))
                assert np.all(dm <= 4.5 * 1.2533 * se + floor), (name, scan, s, "medians", np.median(ref, axis=0), np.median(gpu, axis=0), se)
            d = np.abs(ref.mean(axis=0) - gpu.mean(axis=0))
            assert np.all(d <= 4.5 * se + loose), (name, scan, s, "means", ref.mean(axis=0), gpu.mean(axis=0), se)
        # Allowances on top of the combined standard error: what the data uses (tools/f5_margins.py, profiles/r03_f5_margins.json)
        # is nothing at all for the toric, rotated and biased L = 7 ladders; the biased xzzx L = 5 ladder needs 0.015 on the
        # class-histogram means (1 GPU replica in 9 sits in a mode the reference's 16 never visited) and < 1e-3 elsewhere.
        # The sharp pins of these paths are the exact enumerations of test_gpu_stats.py (5 sigma, 4096 replicas).
        # scan = "wave" takes the same allowances.
        if wave:
            st = b["states"]
            nerr = np.stack([tm.count_errors(np.ascontiguousarray(st[:, c])) if code == q.TORIC else np.count_nonzero(st[:, c].reshape(R, -1), axis=1)
                             for c in range(Nc)], axis=1).astype(np.float64)                   # [R, Nc] at the final step
            close(r_n, nerr, 0.02, 5e-3 * r_n.mean(axis=0).max(), medians=False)
        else:
            acc = (b["swap_accepts"].astype(np.int64) - a["swap_accepts"]) / win          # [R, Nc-1] acceptance per replica
            nerr = (b["nerr_sums"].astype(np.int64) - a["nerr_sums"]) / win               # [R, Nc]
            close(r_acc, acc, 1e-3, 5e-3)
            close(r_n, nerr, 0.02, 5e-3 * r_n.mean(axis=0).max())
        close(r_h, hist, 5e-3, 0.02)


# ------------------------------------------------------------------ exact chunked continuation
@pytest.mark.parametrize("code_name,L,Nc,eta", [("toric", 5, 5, None), ("rotated", 7, 7, None), ("xzzx", 5, 5, 30.0)])
def test_chunked_continuation_is_one_long_run(q, orc, code_name, L, Nc, eta):
    from qecmc import harness
    rng = np.random.default_rng(4)
    code = harness._CODES[code_name]
    init = rand_states(rng, 80, L, 0.1) if code_name == "toric" else rand_plaq(rng, 80, L, 0.1)
    full = q.pteq_batch(init, 0.12, Nc=Nc, steps=300, iters=10, tops_burn=2, seed=21, first_syndrome=7, code=code, eta=eta, return_states=True)
    run = harness.LadderRun(init, 0.12, Nc=Nc, iters=10, tops_burn=2, seed=21, first_syndrome=7, code=code, eta=eta)
    for chunk in (1, 99, 37, 163):
        run.advance(chunk)
    snap = run.snapshot(states=True)
    assert snap["steps"] == 300
    for k in ("counts", "samples", "tops0", "states"):
        assert np.array_equal(snap[k], full[k]), k


def test_convergence_study_continues_exactly(q):
    from qecmc import harness
    rng = np.random.default_rng(9)
    raw = harness.draw_errors("rotated", 7, 96, 0.12, rng)
    out = harness.convergence_study(raw, 0.12, [100, 400, 1600], Nc=7, seed=4, code=q.ROTATED, chunk=500)
    for i, c in enumerate((100, 400, 1600)):
        one = q.pteq_batch(raw, 0.12, Nc=7, steps=c, iters=10, tops_burn=0, seed=4, code=q.ROTATED)
        assert np.array_equal(out["counts"][i], one["counts"]) and np.array_equal(out["samples"][i], one["samples"])


# ------------------------------------------------------------------ harness: shards, resume, metrics, threshold curve (f1)
def test_shards_resume_bit_for_bit(q, tmp_path):
    from qecmc import harness
    params = {"code": "toric", "size": 5, "p_error": 0.08, "noise": "depolarizing"}
    kw = dict(steps=400, conv_criteria=None, tops_burn=1, metrics="full")
    log = []
    paths = harness.generate_shards(params, 250, 100, str(tmp_path), seed=3, log=log, **kw)
    assert [os.path.basename(p) for p in paths] == [harness.shard_name("data", 3, k) for k in range(3)]
    assert len(log) == 3 and all(os.path.exists(p) for p in paths)
    first = [dict(np.load(p)) for p in paths]
    assert [f["eq_true"].shape[0] for f in first] == [100, 100, 50]
    # metrics line: proposals, rates, swap acceptance per rung pair, tops0 histogram, success rate
    lines = [json.loads(ln) for ln in open(tmp_path / "data_metrics.jsonl")]
    assert len(lines) == 3 and lines[1]["shard"] == 1 and lines[2]["syndromes"] == 50
    assert lines[0]["proposals"] == 100 * 5 * 10 * 400 and len(lines[0]["swap_acceptance"]) == 4 and len(lines[0]["tops0_hist"]) == 21
    assert 0 <= lines[0]["success_rate"] <= 1 and lines[0]["chain_sweeps_per_s_kernel"] > 0
    # resume: delete one shard, run again -> only that one is remade, bit for bit; the others are untouched
    mt = [os.path.getmtime(p) for p in paths]
    os.remove(paths[1])
    log2 = []
    harness.generate_shards(params, 250, 100, str(tmp_path), seed=3, log=log2, **kw)
    assert [ln["shard"] for ln in log2] == [1]
    again = dict(np.load(paths[1]))
    assert all(np.array_equal(again[k], first[1][k]) for k in first[1])
    assert os.path.getmtime(paths[0]) == mt[0] and os.path.getmtime(paths[2]) == mt[2]
    # a shard does not depend on which other shards were made: shard 2 alone in a fresh directory
    solo = harness.generate(params, 50, seed=3, rng=np.random.default_rng([3, 2]), first_syndrome=200, **kw)
    assert np.array_equal(solo["counts"], first[2]["counts"]) and np.array_equal(solo["qubit_matrix"], first[2]["qubit_matrix"])


def test_threshold_curve(q):
    """p in [0.05, 0.20] (generate_data.py's scan): the success rate falls with p.  (Fixed-length runs: a syndrome whose ladder
    has not passed the tops0 burn-in returns an all-zero distribution -- argmax 0 -- exactly as the reference's PTEQ does, which
    bounds the success rate at low p where tops are rare.)"""
    from qecmc import harness
    params = {"code": "toric", "size": 5, "noise": "depolarizing"}
    out = harness.threshold_curve(params, [0.05, 0.10, 0.15, 0.20], 512, seed=1, steps=20000, conv_criteria=None, tops_burn=1)
    assert out["success_rate"].shape == (4,) and np.all(out["err"] < 0.03)
    assert out["success_rate"][0] > 0.75 and out["success_rate"][0] > out["success_rate"][3] + 5 * out["err"][3]
    assert np.all(np.diff(out["success_rate"][1:]) < 3 * out["err"][2:] + 0.02)        # non-increasing within error (past the burn-in bound at p = 0.05)
    assert len(out["metrics"]) == 4 and out["metrics"][3]["frac_past_burn_in"] > 0.5
    # beside the raw rate: the rate among the syndromes whose ladder got past the burn-in (the trap is not the decoder's failure)
    assert np.all(out["frac_sampled"] > 0.5) and np.all(out["success_rate_sampled"] >= out["success_rate"] - 1e-12)


def test_generate_with_criterion_takes_the_work_queue(q, orc):
    """harness.generate(conv_criteria='error_based') -- the reference's default route -- must run on the work-queue kernels
    (per-batch mixing counters used to switch them off).  With the persistent grid forced to one workgroup every lane
    runs several ladders; results equal the oracle's one run per syndrome, and metrics='full' (which cannot use the queue)
    gives the same answers from the one-ladder-per-lane kernel."""
    from qecmc import harness
    params = {"code": "toric", "size": 3, "p_error": 0.1, "noise": "depolarizing", "Nc": 3}
    kw = dict(steps=1500, conv_criteria="error_based", tops_burn=2, SEQ=2, TOPS=6, eps=0.3, iters=5)
    a = harness.generate(params, 333, seed=9, flags=q.dev_flags(queue_grid=1), **kw)
    assert "swap_acceptance" not in a["metrics"]
    b = harness.generate(params, 333, seed=9, metrics="full", **kw)
    assert "swap_acceptance" in b["metrics"]
    for k in ("counts", "steps_done", "converged", "samples", "tops0"):
        assert np.array_equal(a[k], b[k]), k
    assert a["converged"].any() and np.unique(a["steps_done"]).size > 10          # lanes did finish at different steps and refill


# ------------------------------------------------------------------ work queue for runs that stop by the criterion (f3)
@pytest.mark.parametrize("L,p,Nc,N,steps,iters,grid,kw", [
    (3, 0.10, 3, 300, 3000, 10, 1, dict(tops_burn=1, SEQ=1, TOPS=4, eps=0.5)),        # one workgroup eats 300 ladders
    (3, 0.10, 3, 333, 1500, 5, 2, dict(tops_burn=2, SEQ=2, TOPS=6, eps=0.3)),         # iters = 5: ladders may start every 4th step only
    (5, 0.10, 5, 200, 8000, 8, 1, dict(tops_burn=1, SEQ=1, TOPS=3, eps=0.8)),         # iters = 8: any step
    (3, 0.12, 3, 150, 400, 10, 1, dict(tops_burn=1, SEQ=1, TOPS=4, eps=0.5)),         # short horizon: many ladders end unconverged
    (9, 0.15, 8, 140, 300, 10, 1, dict(tops_burn=0, SEQ=0, TOPS=0, eps=0.05)),        # the headline shape (dE table); ladders of a few steps each
    (3, 0.2, 2, 130, 500, 10, 0, dict(tops_burn=0, SEQ=0, TOPS=1, eps=1.0))])         # grid 0: the production grid (no refill needed)
def test_work_queue_bit_exact(q, orc, L, p, Nc, N, steps, iters, grid, kw):
    """A finished lane takes the next ladder of the batch in place; with the persistent grid forced down to one or two
    workgroups every lane runs several ladders one after the other.  Every ladder must come out as the oracle's single run."""
    rng = np.random.default_rng(L * 100 + N)
    init = rand_states(rng, N, L, p)
    kw = dict(kw, steps=steps, iters=iters, seed=99, first_syndrome=5, conv_criteria="error_based")
    got = q.pteq_batch(init, p, Nc=Nc, flags=q.dev_flags(queue_grid=grid), **kw)
    ref = orc.toric_pteq_batch(init, p, Nc, kw.pop("steps"), **kw)
    assert np.array_equal(got["converged"], ref["converged"])
    assert np.array_equal(got["steps_done"], ref["steps_done"].astype(np.uint32))
    assert np.array_equal(got["samples"], ref["samples"].astype(np.uint32))
    assert np.array_equal(got["tops0"], ref["tops0"].astype(np.uint32))
    assert np.array_equal(got["counts"], ref["counts"])
    assert got["converged"].any()
    if steps == 400:
        assert not got["converged"].all()                                              # the horizon ended some


def test_work_queue_with_replicas(q, orc):
    rng = np.random.default_rng(77)
    init = rand_states(rng, 20, 3, 0.1)
    R = 9
    kw = dict(tops_burn=2, seed=4, conv_criteria="error_based", TOPS=6, SEQ=2, eps=0.2)
    got = q.pteq_batch(init, 0.1, Nc=3, steps=4000, replicas=R, flags=q.dev_flags(queue_grid=1), **kw)
    ref = orc.toric_pteq_batch(np.repeat(init, R, axis=0), 0.1, 3, 4000, **kw)
    assert np.array_equal(got["counts"], ref["counts"].reshape(20, R, 16).sum(axis=1))
    assert np.array_equal(got["steps_done"], ref["steps_done"].reshape(20, R).max(axis=1).astype(np.uint32))
    assert np.array_equal(got["converged"], ref["converged"].reshape(20, R).all(axis=1))


# ------------------------------------------------------------------ top-chain Philox blocks drawn ahead (PRE instantiations)
@pytest.mark.parametrize("name,L,Nc,iters,steps,N", [
    ("toric", 15, 8, 10, 30, 70), ("toric", 15, 8, 13, 12, 40), ("toric", 15, 8, 3, 40, 40), ("toric", 15, 8, 1, 50, 20),
    ("toric", 15, 3, 10, 20, 33), ("toric", 15, 15, 10, 12, 20), ("toric", 13, 8, 7, 25, 30), ("toric", 16, 9, 10, 10, 10),
    ("toric", 15, 8, 30, 8, 20), ("toric", 15, 8, 27, 9, 20),          # more proposals than the 12 two-proposal blocks kept; an odd count
    ("rotated", 21, 8, 10, 20, 40), ("rotated", 21, 3, 5, 20, 20), ("rotated", 21, 12, 10, 8, 10), ("xzzx", 19, 8, 10, 12, 20)])
def test_top_blocks_drawn_ahead_bit_exact(q, orc, name, L, Nc, iters, steps, N):
    """Shapes whose LDS footprint leaves 4 waves per SIMD take the instantiations in which the wave that will be the top chain
    draws that step's Philox blocks one and two steps earlier (half each): more or fewer proposals than the 12 blocks kept,
    odd halves, three-rung ladders, 960-thread workgroups, the plaquette codes' framed top chain."""
    rng = np.random.default_rng(L * 7 + Nc + iters)
    if name == "toric":
        init = rand_states(rng, N, L, 0.15)
        got = q.pteq_batch(init, 0.15, Nc=Nc, steps=steps, iters=iters, tops_burn=0, seed=31, first_syndrome=9, return_states=True)
        ref = orc.toric_pteq_batch(init, 0.15, Nc, steps, iters=iters, tops_burn=0, seed=31, first_syndrome=9, return_states=True)
    else:
        code, ocode = (q.ROTATED, orc.ROTATED) if name == "rotated" else (q.XZZX, orc.XZZX)
        init = rand_plaq(rng, N, L, 0.15)
        got = q.pteq_batch(init, 0.15, Nc=Nc, steps=steps, iters=iters, tops_burn=0, seed=31, first_syndrome=9, return_states=True, code=code)
        ref = orc.pteq_batch(ocode, init, 0.15, Nc, steps, iters=iters, tops_burn=0, seed=31, first_syndrome=9, return_states=True)
    assert np.array_equal(got["states"], ref["states"])
    assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["tops0"], ref["tops0"].astype(np.uint32))


def test_top_blocks_drawn_ahead_across_chunks(q):
    """Every launch starts without blocks in hand (its first two top steps draw in place): chunked continuation stays exact."""
    from qecmc import harness
    rng = np.random.default_rng(12)
    init = rand_states(rng, 40, 15, 0.15)
    full = q.pteq_batch(init, 0.18, Nc=8, steps=23, iters=10, tops_burn=0, seed=8, return_states=True)
    run = harness.LadderRun(init, 0.18, Nc=8, iters=10, tops_burn=0, seed=8)
    for chunk in (1, 2, 5, 3, 12):
        run.advance(chunk)
    snap = run.snapshot(states=True)
    assert np.array_equal(snap["states"], full["states"]) and np.array_equal(snap["counts"], full["counts"])


@pytest.mark.parametrize("name,L,Nc,N,steps,iters", [("rotated", 5, 5, 200, 3000, 10), ("xzzx", 5, 4, 150, 2000, 8), ("planar", 5, 5, 140, 2500, 10),
                                                     ("rotated", 7, 3, 100, 1500, 5)])
def test_work_queue_plaquette_codes_bit_exact(q, orc, name, L, Nc, N, steps, iters):
    rng = np.random.default_rng(L * 11 + N)
    code, ocode = {"rotated": (q.ROTATED, orc.ROTATED), "xzzx": (q.XZZX, orc.XZZX), "planar": (q.PLANAR, orc.PLANAR)}[name]
    if name == "planar":
        init = rand_states(rng, N, L, 0.1)
        init[:, 1, -1, :] = 0; init[:, 1, :, -1] = 0
    else:
        init = rand_plaq(rng, N, L, 0.12)
    kw = dict(steps=steps, iters=iters, tops_burn=1, seed=17, first_syndrome=3, conv_criteria="error_based", SEQ=1, TOPS=4, eps=0.5)
    got = q.pteq_batch(init, 0.12, Nc=Nc, code=code, flags=q.dev_flags(queue_grid=1), **kw)
    ref = orc.pteq_batch(ocode, init, 0.12, Nc, kw.pop("steps"), **kw)
    for k in ("converged", "steps_done", "samples", "tops0"):
        assert np.array_equal(got[k], ref[k].astype(got[k].dtype)), k
    assert np.array_equal(got["counts"], ref["counts"])
    assert got["converged"].any() or L == 7          # (the three-rung L = 7 ladders all run to the horizon: refills by horizon only)


@pytest.mark.parametrize("name,L,Nc,N,steps,iters,eta,alpha", [
    ("xzzx", 5, 5, 200, 3000, 10, 100.0, None), ("rotated", 5, 4, 150, 2000, 8, 10.0, None), ("xzzx", 7, 3, 100, 1500, 5, 30.0, None),
    ("xzzx", 5, 5, 200, 3000, 10, None, 1.7), ("rotated", 5, 4, 140, 2500, 10, None, 2.5), ("xzzx", 3, 2, 90, 1200, 6, None, 1.2)])
def test_work_queue_biased_and_alpha_bit_exact(q, orc, name, L, Nc, N, steps, iters, eta, alpha):
    """The work queue under the biased and alpha rules (what generate_data.py:142-150 routes biased noise to: PTEQ_alpha with the
    error_based criterion): the grid forced to one workgroup, every lane runs several ladders; each must come out as the oracle's
    single run -- counts, samples, tops0, stopping step, flag."""
    rng = np.random.default_rng(L * 13 + N)
    code, ocode = {"rotated": (q.ROTATED, orc.ROTATED), "xzzx": (q.XZZX, orc.XZZX)}[name]
    init = rand_plaq(rng, N, L, 0.12)
    kw = dict(steps=steps, iters=iters, tops_burn=1, seed=23, first_syndrome=7, conv_criteria="error_based", SEQ=1, TOPS=4, eps=0.5)
    p = 0.12 if eta is not None else 0.1
    noise = dict(eta=eta) if eta is not None else dict(alpha=alpha)
    got = q.pteq_batch(init, p, Nc=Nc, code=code, flags=q.dev_flags(queue_grid=1), **noise, **kw)
    okw = dict(noise=orc.BIASED, eta=eta) if eta is not None else dict(noise=orc.ALPHA, alpha=alpha, det_pow=1)
    ref = orc.pteq_batch(ocode, init, p, Nc, kw.pop("steps"), **okw, **kw)
    for k in ("converged", "steps_done", "samples", "tops0"):
        assert np.array_equal(got[k], ref[k].astype(got[k].dtype)), k
    assert np.array_equal(got["counts"], ref["counts"])
    assert got["converged"].any() and np.unique(got["steps_done"]).size > 5


# ------------------------------------------------------------------ syndrome generation on the device (row f1)
@pytest.mark.parametrize("name,L,rates,N,first", [("toric", 9, (0.05, 0.05, 0.05), 1000, 0), ("toric", 4, (0.1, 0.1, 0.1), 77, 4000),
                                                  ("xzzx", 9, (7.4257e-4, 7.4257e-4, 0.148515), 600, 12), ("rotated", 21, (0.17 / 3,) * 3, 65, 1),
                                                  ("planar", 5, (0.03, 0.04, 0.05), 300, 0), ("xzzx", 3, (0.3, 0.0, 0.2), 50, 9)])
def test_generate_syndromes_bit_exact(q, orc, name, L, rates, N, first):
    from qecmc import harness
    code, ocode = {"toric": (q.TORIC, orc.TORIC), "xzzx": (q.XZZX, orc.XZZX), "rotated": (q.ROTATED, orc.ROTATED), "planar": (q.PLANAR, orc.PLANAR)}[name]
    for hide in (True, False):
        init, raw, eq = harness.generate_syndromes(code, L, N, rates=rates, hide=hide, seed=77, first_syndrome=first)
        ri, rr, re = orc.generate_syndromes(ocode, L, N, *rates, hide_class=hide, seed=77, first_syndrome=first)
        assert np.array_equal(raw, rr) and np.array_equal(eq, re) and np.array_equal(init, ri)
        assert hide or np.array_equal(init, raw)


def test_generate_syndromes_validation_and_harness(q):
    from qecmc import harness, _lib as L_
    import ctypes as C
    out = np.zeros((4, 2, 5, 5), dtype=np.uint8)
    rc = L_.lib().qecmc_generate_syndromes(L_.TORIC, 5, 4, 0.1, 0.05, 0.05, 1, 0, 0, L_.u8(out), None, None)
    assert rc == -1 and b"p_x = p_y = p_z" in L_.lib().qecmc_last_error()
    assert L_.lib().qecmc_generate_syndromes(L_.XZZX, 5, 4, 0.6, 0.3, 0.3, 1, 0, 0, L_.u8(out), None, None) == -1
    assert L_.lib().qecmc_generate_syndromes(L_.TORIC, 5, 4, 0.05, 0.05, 0.05, 1, 0, 0, L_.u8(out), None, None) == 0      # nullable outputs
    # the batched recipe with the errors drawn on the GPU: low noise decodes, shards do not depend on the cut
    params = {"code": "rotated", "size": 5, "p_error": 0.05, "noise": "depolarizing"}
    a = harness.generate(params, 200, seed=3, steps=3000, conv_criteria=None, tops_burn=0, device_generation=True)
    assert a["success"].mean() > 0.9
    b = harness.generate(params, 100, seed=3, steps=3000, conv_criteria=None, tops_burn=0, device_generation=True, first_syndrome=100)
    assert np.array_equal(b["qubit_matrix"], a["qubit_matrix"][100:]) and np.array_equal(b["counts"], a["counts"][100:])


# ------------------------------------------------------------------ regressions found by tests/fuzz_gpu.py
@pytest.mark.parametrize("L,Nc,noise", [(17, 1, "alpha"), (17, 1, "biased"), (21, 1, "biased"), (21, 2, "alpha"), (19, 3, "biased")])
def test_xzzx_logical_product_rows_small_workgroups(q, orc, L, Nc, noise):
    """The biased / alpha kernels keep the xzzx code's four logical-operator products (I, X, Z, XZ) as 4 W mask words in LDS.  A
    1-rung ladder has 64 threads, fewer than 4 W from L = 17 on: the rows must be filled by a strided loop (found by the
    randomised sweep: xzzx L = 17, Nc = 1, alpha noise)."""
    rng = np.random.default_rng(L + Nc)
    init = rand_plaq(rng, 70, L, 0.2)
    kw = dict(steps=120, iters=10, tops_burn=0, seed=661175579, first_syndrome=484)
    if noise == "alpha":
        got = q.pteq_batch(init, 0.3, Nc=Nc, code=q.XZZX, alpha=1.3, return_states=True, **kw)
        ref = orc.pteq_batch(orc.XZZX, init, 0.3, Nc, kw["steps"], iters=10, tops_burn=0, seed=kw["seed"], first_syndrome=484,
                             noise=orc.ALPHA, alpha=1.3, det_pow=1, return_states=True)
    else:
        got = q.pteq_batch(init, 0.15, Nc=Nc, code=q.XZZX, eta=10.0, return_states=True, **kw)
        ref = orc.pteq_batch(orc.XZZX, init, 0.15, Nc, kw["steps"], iters=10, tops_burn=0, seed=kw["seed"], first_syndrome=484,
                             noise=orc.BIASED, eta=10.0, return_states=True)
    assert np.array_equal(got["states"], ref["states"]) and np.array_equal(got["counts"], ref["counts"])


@pytest.mark.parametrize("name,iters,eta", [("xzzx", 64, 100.0), ("rotated", 100, 10.0), ("xzzx", 10, 1e6)])
def test_biased_fast_test_precision_fallback(q, orc, name, iters, eta):
    """The biased rule's fast test runs in single precision while 4 iters max|log2 ratio| <= 2000 and in fp64 beyond (many proposals per
    step, extreme bias): both sides of the switch stay bit-identical to the oracle."""
    rng = np.random.default_rng(iters)
    L, Nc = 5, 4
    init = rand_plaq(rng, 90, L, 0.12)
    code, ocode = (q.XZZX, orc.XZZX) if name == "xzzx" else (q.ROTATED, orc.ROTATED)
    kw = dict(steps=60, iters=iters, tops_burn=0, seed=4242, first_syndrome=7)
    got = q.pteq_batch(init, 0.12, Nc=Nc, code=code, eta=eta, return_states=True, **kw)
    ref = orc.pteq_batch(ocode, init, 0.12, Nc, kw["steps"], iters=iters, tops_burn=0, seed=4242, first_syndrome=7, noise=orc.BIASED, eta=eta,
                         return_states=True)
    assert np.array_equal(got["states"], ref["states"]) and np.array_equal(got["counts"], ref["counts"])
