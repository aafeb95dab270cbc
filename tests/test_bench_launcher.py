"""`bench.py --gpus N` must start N ranks itself.  Rehearsed on CPU: the same launcher command line
(python -m torch.distributed.run --nproc-per-node N bench.py --gpus N), gloo instead of RCCL and no kernel (`--dry-run`),
so what is checked is the launch path, the rank environment, the gather and the JSON contract -- not a throughput."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*argv, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=300, env=e)


def test_bench_gpus2_spawns_two_ranks():
    r = _run("--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1", "--syndromes", "256")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                      # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert out["gather_ok"] is True                       # rank 1's records reached rank 0
    # the line certifies its own ranks: the communicator's world and backend, one record per rank with its shard's first syndrome
    assert out["comm"] == {"backend": "gloo", "world": 2}
    assert [r["rank"] for r in out["ranks"]] == [0, 1]
    assert [r["first_syndrome"] for r in out["ranks"]] == [0, 256]
    assert all("device" in r and "kernel_ms_mean" in r for r in out["ranks"])
    assert out["value"] == 0.0 and "dry run" in out["metric"]          # a rehearsal never reports a throughput


def test_bench_single_rank_dry_run_and_rc_propagation():
    r = _run("--dry-run", "--steps", "1", "--warmup", "0", "--syndromes", "64", "--config", "4")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and "XZZX" in out["config"]["workload"]
    # a failing rank must fail the launcher: without --dry-run there is no GPU here, every rank raises
    r = _run("--gpus", "2", "--steps", "1", "--warmup", "0", "--syndromes", "64")
    assert r.returncode != 0


def test_bench_rejects_mismatched_world():
    r = _run("--gpus", "2", "--dry-run", env={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def _sharded_oracle(rank, world, n_total):
    """module-level (picklable) rank function for sharding.launch: the sharded call with the oracle as stand-in compute"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_shard_gloo import _oracle_compute
    from qecmc.sharding import pteq_batch_sharded
    rng = np.random.default_rng(5)
    init = np.zeros((n_total, 2, 3, 3), dtype=np.uint8)
    err = rng.random(init.shape) < 0.15
    init[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    out = pteq_batch_sharded(init, 0.1, compute=_oracle_compute, Nc=3, steps=40, tops_burn=0, seed=7)
    if rank != 0:
        return None
    full = _oracle_compute(init, 0.1, Nc=3, steps=40, tops_burn=0, seed=7)
    return bool(all(np.array_equal(out[k], full[k].astype(np.uint32)) for k in ("counts", "samples", "tops0"))), world


def test_sharding_launch_helper_gloo():
    sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
    from qecmc.sharding import launch
    ok, world = launch(2, _sharded_oracle, args=(9,), backend="gloo", timeout=120)
    assert ok is True and world == 2


def _failing(rank, world):
    if rank == 1:
        raise SystemExit(3)
    return 1


def test_sharding_launch_propagates_failure():
    sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
    from qecmc.sharding import launch
    with pytest.raises(RuntimeError):
        launch(2, _failing, backend="gloo", timeout=60)


@pytest.mark.gpu
def test_bench_under_torchrun_initialises_rccl_and_gathers():
    """The driver's launcher form on the GPU box, world 1, as a FRESH child process: RCCL initialises, the gather
    path runs, the line certifies its communicator and its rank's shard."""
    from qecmc.sharding import free_port
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
           "--ladder-steps", "500"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert "nccl" in out["comm"]["backend"] and out["comm"]["world"] == 1
    assert out["ranks"][0]["first_syndrome"] == 0 and out["n_gpus"] == 1 and out["value"] > 0


def test_bench_argument_defaults_of_the_criterion_and_alpha_routes():
    """What the bench modes resolve to without a GPU: the default line is BASELINE config 2 on the scan = wave kernels; --criterion runs 8 ladders per lane of
    the persistent grid to a horizon of 262 144; --alpha-route decodes biased xzzx noise with PTEQ_alpha's (pz_tilde, alpha) of generate_data.py:145-146;
    `--scan auto` follows the same-box A/B runs (profiles/r04_wave_ab.json)."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args([])
    assert (a.code, a.L, a.Nc, a.syndromes, a.ladder_steps, a.scan, a.steps, a.warmup) == ("toric", 9, 8, 65536, 10000, "wave", 5, 1)
    c = bench.parse_args(["--criterion"])
    assert (c.syndromes, c.ladder_steps, c.steps, c.warmup, c.scan) == (524288, 262144, 2, 0, "wave")
    al = bench.parse_args(["--alpha-route", "--criterion"])
    assert (al.code, al.L, al.Nc, al.eta, al.syndromes, al.ladder_steps, al.scan) == ("xzzx", 5, 5, 100.0, 16 * 98304, 65536, "wave")
    pz, alpha = bench.rule(al)
    assert abs(pz - (0.15 / (1 + 1 / 100.0)) / 0.85) < 1e-15 and abs(alpha - np.log(pz / 200.0) / np.log(pz)) < 1e-12
    assert bench.parse_args(["--config", "3"]).scan == "wave" and bench.parse_args(["--config", "3", "--criterion"]).scan == "random"
    assert bench.parse_args(["--config", "4"]).scan == "random" and bench.parse_args(["--config", "5"]).scan == "random"
    assert bench.parse_args(["--config", "2", "--code", "xzzx"]).scan == "wave" and bench.parse_args(["--config", "2", "--code", "xzzx", "--iters", "7"]).scan == "random"
    assert bench.parse_args(["--syndromes", "1000"]).scan == "random"
    assert bench.parse_args(["--iters", "7"]).scan == "random" and bench.parse_args(["--iters", "7", "--Nc", "9"]).scan == "wave"


def test_bench_steps_are_what_the_caller_asked_for():
    """--steps / --warmup are taken as given in every mode (a criterion run's own defaults apply only when neither is given)"""
    sys.path.insert(0, ROOT)
    import bench
    for extra in ([], ["--criterion"], ["--alpha-route", "--criterion"]):
        a = bench.parse_args(extra + ["--steps", "5", "--warmup", "1"])
        assert (a.steps, a.warmup) == (5, 1)
        a = bench.parse_args(extra + ["--steps", "7", "--warmup", "0"])
        assert (a.steps, a.warmup) == (7, 0)
    assert (bench.parse_args(["--criterion", "--steps", "3"]).warmup, bench.parse_args(["--steps", "3"]).warmup) == (1, 1)
    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_bench_dump_outputs_exact_and_bounded(tmp_path):
    """--dump-outputs: u32 records as exact float64; above the cap every array keeps the same seeded rows, listed in rows.npy"""
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(1)
    small = dict(counts=rng.integers(0, 2**32, (100, 16), dtype=np.uint32), samples=np.arange(100, dtype=np.uint32))
    bench.dump_outputs(str(tmp_path / "a"), small)
    got = np.load(tmp_path / "a" / "counts.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint64), small["counts"].astype(np.uint64))
    assert not (tmp_path / "a" / "rows.npy").exists()
    n = 600000                                                   # 600 000 x (16 + 2) x 8 B = 86 MB > 64 MB
    big = dict(counts=np.tile(np.arange(n, dtype=np.uint32)[:, None], (1, 16)), samples=np.arange(n, dtype=np.uint32),
               tops0=np.arange(n, dtype=np.uint32))
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
    total = sum(os.path.getsize(p) for p in (tmp_path / "b").iterdir())
    assert total <= 64 << 20
    rows = np.load(tmp_path / "b" / "rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "c" / "rows.npy")) and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "samples.npy"), rows) and np.array_equal(np.load(tmp_path / "b" / "counts.npy")[:, 3], rows)


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_timed_path_results(tmp_path):
    """A plain run with --dump-outputs, in a fresh child process: the files hold the last timed step's class counts, samples and tops0,
    equal to the CPU oracle's on the same Philox streams; the line carries no --full companion."""
    sys.path.insert(0, ROOT)
    import bench
    # (3000 ladder steps: long enough that the oracle's rows are not all zero -- at a few hundred no ladder passes the burn-in)
    argv = ["--steps", "2", "--warmup", "1", "--syndromes", "4096", "--ladder-steps", "3000"]
    r = _run(*argv, "--dump-outputs", str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert not {"cpu_baseline", "histogram_match", "random_scan", "ms_per_step_incl_transfers"} & set(out)
    got = {k: np.load(tmp_path / (k + ".npy")) for k in ("counts", "samples", "tops0")}
    assert got["counts"].shape == (4096, 16) and all(v.dtype == np.float64 for v in got.values())
    a = bench.parse_args(argv)
    init = bench.make_batch(a, 0)[:64]
    ref = bench.oracle_batch(a, init, a.ladder_steps, 16)
    assert ref["counts"].sum() > 0 and (ref["samples"] > 0).any() and (ref["tops0"] > 0).any()      # a comparison that can fail
    for k in ("counts", "samples", "tops0"):
        assert np.array_equal(got[k][:64].astype(np.uint64), np.asarray(ref[k]).astype(np.uint64)), k
