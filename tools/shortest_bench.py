#!/usr/bin/env python3
"""Timings of the in-kernel shortest-chain statistics (qecmc.pteq_shortest_batch) -> profiles/r08_shortest.json

  (a) one syndrome, xzzx L = 9, Nc = 9, alpha = 2, pz_tilde = 0.15, 20 000 fixed ladder steps: PTEQ_alpha_with_shortest on the host loop (scan="random", the
      parent commit's only form, unchanged here) against scan="colour" and scan="wave"; alternated, `--repeats` each after a warm-up; ladder steps per second
  (b) 65 536 xzzx L = 9 syndromes, Nc = 8, 2 000 fixed steps: kernel time (device events) of pteq_shortest_batch(scan="wave") against plain
      pteq_batch(alpha, scan="wave"); the ratio is the price of the key and the set

    tools/shortest_bench.py [--repeats 5] [--batch 65536] [--out profiles/r08_shortest.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "mcmc-qec-toric-rl_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps-one", type=int, default=20000)
    ap.add_argument("--steps-batch", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import qecmc
    rng = np.random.default_rng(9)
    L, pz, alpha = 9, 0.15, 2.0
    code = qecmc.xzzx_code(L)
    code.qubit_matrix = (rng.integers(1, 4, (L, L)) * (rng.random((L, L)) < 0.1)).astype(np.uint8)
    kw = dict(Nc=9, steps=args.steps_one, iters=10, conv_criteria=None, tops_burn=2, seed=5)
    routes = ("random", "colour", "wave")
    for scan in routes:                                                   # warm-up: library load, plan cache, first launch
        qecmc.PTEQ_alpha_with_shortest(code, pz, alpha, scan=scan, **dict(kw, steps=200))
    one = {scan: [] for scan in routes}
    for _ in range(args.repeats):
        for scan in routes:
            t0 = time.perf_counter()
            qecmc.PTEQ_alpha_with_shortest(code, pz, alpha, scan=scan, **kw)
            one[scan].append(args.steps_one / (time.perf_counter() - t0))
    res_a = {scan: dict(steps_per_s=v, median=float(np.median(v)), spread=float(max(v) - min(v))) for scan, v in one.items()}
    for scan in ("colour", "wave"):
        res_a[scan]["ratio_to_host_loop"] = res_a[scan]["median"] / res_a["random"]["median"]
        res_a[scan]["beats_host_loop_by_more_than_the_spread"] = bool(min(one[scan]) - max(one["random"]) > max(res_a[scan]["spread"], res_a["random"]["spread"]))
    print("(a)", json.dumps({k: (round(v["median"]), round(v["spread"])) for k, v in res_a.items()}), flush=True)

    N = args.batch
    init = (rng.integers(1, 4, (N, L, L)) * (rng.random((N, L, L)) < 0.1)).astype(np.uint8)
    bkw = dict(Nc=8, steps=args.steps_batch, iters=10, tops_burn=2, seed=5, code=qecmc.XZZX, scan="wave", return_stats=True)
    plain, short = [], []
    qecmc.pteq_batch(init[:4096], pz, alpha=alpha, **bkw)
    qecmc.pteq_shortest_batch(init[:4096], pz, alpha, **bkw)
    for _ in range(3):
        plain.append(qecmc.pteq_batch(init, pz, alpha=alpha, **bkw)["stats"]["kernel_ms"])
        r = qecmc.pteq_shortest_batch(init, pz, alpha, **bkw)
        short.append(r["stats"]["kernel_ms"])
    res_b = dict(batch=N, steps=args.steps_batch, plain_alpha_wave_kernel_ms=plain, shortest_wave_kernel_ms=short,
                 ratio=float(np.median(short) / np.median(plain)), overflowed=int(r["overflow"].sum()))
    print("(b)", json.dumps(res_b), flush=True)
    out = dict(command=" ".join(["tools/shortest_bench.py"] + sys.argv[1:]), one_syndrome=dict(shape="xzzx L=9 Nc=9 alpha=2 pz_tilde=0.15", steps=args.steps_one, **res_a),
               batch=dict(shape="xzzx L=9 Nc=8 alpha=2 pz_tilde=0.15", **res_b))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
