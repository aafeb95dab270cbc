#!/usr/bin/env python3
"""Kernel times of the exact marginals (qecmc_class_marginals) next to the sweep they extend -> profiles/class_marginal_rate.json.

    GPU box:  rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/class_marginal_rate.py --trace
    anywhere: python3 tools/class_marginal_rate.py --summarise OUT/<host>/<pid>_kernel_trace.csv [--out profiles/class_marginal_rate.json]

Per case -- rotated L = 5 (N = 64), L = 9 (N = 32) and L = 11 (N = 8): a job per (syndrome, class); toric L = 5 (N = 1): held generators, 2^8 jobs
per class across several workspace launches --: qecmc_class_marginals and qecmc_class_sweep_cut on the same chains, from this build, in the same
process, alternating: one warm pair, then CALLS pairs.  A call of qecmc_class_sweep at rotated L = 3 separates the warm calls from the timed ones and
one case from the next in the trace (k_class_sweep: a kernel neither entry point launches).  The summary adds up the dispatches per kernel of each
timed segment: the forward, backward, fold and combine kernels against k_class_sweep_cut at the same shape and the same number of workgroups (a job
is one workgroup of the sweep).  No GPU: the tracing form fails."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = [("rotated", 5, 64), ("rotated", 9, 32), ("rotated", 11, 8), ("toric", 5, 1)]
CALLS = 3
P = 0.1
KERNELS = ("k_class_sweep_cut", "k_class_marginal_fwd", "k_class_marginal_bwd", "k_class_marginal_fold", "k_class_marginal_combine")
NOTE = ("rocprofv3 --kernel-trace; *_us: the dispatches of one call added up, mean of %d calls after a warm one, qecmc_class_marginals (depolarizing p = %g) and "
        "qecmc_class_sweep_cut alternating on the same chains; k_class_sweep_cut runs in the latter alone, with one workgroup per job of the former" % (CALLS, P))


def trace():
    import qecmc
    from class_sweep_rate import random_chains
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the times are measured on the device or not at all")
    w4 = qecmc.depolarizing_w4(P)
    mark = lambda: qecmc.class_sweep("rotated", np.zeros((1, 3, 3), np.uint8), w4)
    mark()
    for name, L, n in CASES:
        chains = random_chains(name, L, n)
        for timed in (0, 1):
            for _ in range(CALLS if timed else 1):
                r = qecmc.class_marginals(name, chains, w4=w4)
                z = qecmc.class_sweep_cut(name, chains, w4)["Z"]
                assert r["z"].tobytes() == z.tobytes() and np.allclose(r["marginals"].sum(axis=-1), 1.0)
            mark()


def summarise(path, out):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    segments, cur = [], None
    for r in rows:
        name, ns = r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if "k_class_sweep(" in name or name.rstrip().endswith("k_class_sweep"):
            cur = {}
            segments.append(cur)
        elif cur is not None:
            for k in KERNELS:
                if k + "(" in name or k + "_site(" in name or name.endswith(k):
                    e = cur.setdefault(k, [0.0, 0])
                    e[0] += ns / 1e3
                    e[1] += 1
    segments = segments[:-1]                                                    # (the last marker opens nothing)
    assert len(segments) == 2 * len(CASES), len(segments)
    from qecmc.exact import sweep_cut_info
    cases = []
    for i, (name, L, n) in enumerate(CASES):
        inf = sweep_cut_info(name, L, 0)
        seg = segments[2 * i + 1]                                               # (the warm segment left out)
        us = {k: seg[k][0] / CALLS for k in KERNELS}
        launches = {k: seg[k][1] // CALLS for k in KERNELS}
        jobs = (n * inf["ncls"]) << inf["held"]
        row = dict(code=name, L=L, N=n, width=inf["width"], held=inf["held"], jobs=jobs, sweep_cut_us=us["k_class_sweep_cut"], fwd_us=us["k_class_marginal_fwd"],
                   bwd_us=us["k_class_marginal_bwd"], fold_us=us["k_class_marginal_fold"], combine_us=us["k_class_marginal_combine"],
                   fwd_launches=launches["k_class_marginal_fwd"], sweep_us_per_job=us["k_class_sweep_cut"] / jobs,
                   marginal_us_per_job=(us["k_class_marginal_fwd"] + us["k_class_marginal_bwd"] + us["k_class_marginal_fold"] + us["k_class_marginal_combine"]) / jobs,
                   fwd_over_sweep=us["k_class_marginal_fwd"] / us["k_class_sweep_cut"], bwd_over_sweep=us["k_class_marginal_bwd"] / us["k_class_sweep_cut"],
                   fold_over_sweep=us["k_class_marginal_fold"] / us["k_class_sweep_cut"])
        cases.append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(cases=cases, note=NOTE), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_marginal_rate.json"))
    ap.add_argument("--trace", action="store_true", help="run the alternating calls, for rocprofv3 --kernel-trace")
    ap.add_argument("--summarise", default=None, help="a kernel_trace.csv written by rocprofv3 around a --trace run: write the kernel times into --out")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out)
    elif a.trace:
        trace()
    else:
        ap.error("--trace under rocprofv3, then --summarise")
