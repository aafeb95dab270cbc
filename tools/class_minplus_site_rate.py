#!/usr/bin/env python3
"""Kernel times of the site-cost entry points (qecmc_class_minplus_site, qecmc_class_minplus_chains_site) beside their uniform
siblings in the same run on the same machine -> profiles/class_minplus_site_rate.json.

    GPU box:  rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/class_minplus_site_rate.py --trace
    anywhere: python3 tools/class_minplus_site_rate.py --summarise OUT/<host>/<pid>_kernel_trace.csv [--out profiles/class_minplus_site_rate.json]

Per case -- rotated L = 9 at N = 1 024, rotated L = 11 at N = 64, toric L = 5 at N = 16 -- six calls on the same chains, in this order, one warm round
and then CALLS rounds: qecmc_class_minplus at costs (0, 1, 1, 1); qecmc_class_minplus_site with one table of those costs; the same with a row per
syndrome; qecmc_class_minplus_chains; qecmc_class_minplus_chains_site with one table; with a row per syndrome.  Constant rows, so the six calls do
the same arithmetic on the same entries and return the same results (asserted): what differs is where a CLOSE's cost comes from.  The uniform
kernels are the parent commit's, unchanged: they are the baseline.  The second form adds up the dispatches of every call's kernels, takes the mean
over the CALLS rounds and writes the ratios.  No GPU: the first form fails."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = [("rotated", 9, 1024), ("rotated", 11, 64), ("toric", 5, 16)]
CALLS = 5
ORDER = ["sweep_uniform", "sweep_site_one", "sweep_site_per", "chains_uniform", "chains_site_one", "chains_site_per"]
UNIT = (0, 1, 1, 1)
NOTE = ("kernel_us: rocprofv3 --kernel-trace, the dispatches of one call added up (sweep + reduce; for the chains sweep + pick + reduce + trace + walk), mean of %d "
        "rounds after a warm one; the six calls of a round run on the same chains under constant rows of costs (0, 1, 1, 1), one table (one) and a row per "
        "syndrome (per); *_over_uniform: site kernel time over the uniform sibling's of the same rounds" % CALLS)


def calls_of(name, L, n):
    """the six calls of one case, in ORDER, each returning its result dict"""
    import qecmc
    from class_sweep_rate import random_chains
    chains = random_chains(name, L, n)
    one = np.broadcast_to(np.array(UNIT, np.uint8), chains.shape[1:] + (4,))
    per = np.ascontiguousarray(np.broadcast_to(one, chains.shape + (4,)))
    return [lambda: qecmc.class_minplus(name, chains, UNIT), lambda: qecmc.class_minplus_site(name, chains, one), lambda: qecmc.class_minplus_site(name, chains, per),
            lambda: qecmc.shortest_chains(name, chains, UNIT), lambda: qecmc.shortest_chains_site(name, chains, one),
            lambda: qecmc.shortest_chains_site(name, chains, per)]


def trace():
    import qecmc
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the times are measured on the device or not at all")
    for name, L, n in CASES:
        calls = calls_of(name, L, n)
        for rnd in range(CALLS + 1):                                            # (round 0 warms: code objects, pool blocks, the 128 KiB opt-ins)
            res = [call() for call in calls]
            for r in res[1:3]:
                assert np.array_equal(r["cost"], res[0]["cost"]) and np.array_equal(r["count"], res[0]["count"])
            for r in res[4:]:
                assert np.array_equal(r["chains"], res[3]["chains"]) and np.array_equal(r["cost"], res[3]["cost"])
        print(name, L, n, "traced")


def summarise(path, out):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    mine = [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows if "minplus" in r["Kernel_Name"]]
    is_sweep = lambda k: "k_class_minplus" in k and "k_class_minplus_reduce" not in k
    calls = []                                                                  # every call of these cases is one launch group: it starts with its sweep kernel
    for kernel, ns in mine:
        if is_sweep(kernel):
            calls.append([])
        calls[-1].append((kernel, ns))
    per_case = len(ORDER) * (CALLS + 1)
    assert len(calls) == per_case * len(CASES), (len(calls), per_case)
    res = dict(cases=[], note=NOTE)
    for k, (name, L, n) in enumerate(CASES):
        timed = calls[k * per_case + len(ORDER):(k + 1) * per_case]             # (the warm round left out)
        total, sweep, trace_k = {}, {}, {}
        for i, call in enumerate(timed):
            key = ORDER[i % len(ORDER)]
            site = "site" in key
            assert len(call) == (5 if key.startswith("chains") else 2), (key, call)
            assert all(("_site" in kern) == site for kern, _ in call if is_sweep(kern) or "k_minplus_trace" in kern), (key, call)
            total[key] = total.get(key, 0.0) + sum(ns for _, ns in call) / 1e3 / CALLS
            sweep[key] = sweep.get(key, 0.0) + sum(ns for kern, ns in call if is_sweep(kern)) / 1e3 / CALLS
            trace_k[key] = trace_k.get(key, 0.0) + sum(ns for kern, ns in call if "k_minplus_trace" in kern) / 1e3 / CALLS
        row = dict(code=name, L=L, N=n)
        row.update({"%s_kernel_us" % key: total[key] for key in ORDER})
        row.update({"%s_sweep_kernel_us" % key: sweep[key] for key in ORDER})
        row.update({"%s_trace_kernel_us" % key: trace_k[key] for key in ORDER if key.startswith("chains")})
        for form in ("sweep", "chains"):
            for table in ("one", "per"):
                row["%s_site_%s_over_uniform" % (form, table)] = total["%s_site_%s" % (form, table)] / total["%s_uniform" % form]
        for table in ("one", "per"):
            row["sweep_kernel_site_%s_over_uniform" % table] = sweep["sweep_site_%s" % table] / sweep["sweep_uniform"]
            row["trace_kernel_site_%s_over_uniform" % table] = trace_k["chains_site_%s" % table] / trace_k["chains_uniform"]
        res["cases"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_minplus_site_rate.json"))
    ap.add_argument("--trace", action="store_true", help="run the calls alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--summarise", default=None, help="a kernel_trace.csv written by rocprofv3 around a --trace run: write the kernel times and ratios to --out")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out)
    elif a.trace:
        trace()
    else:
        ap.error("--trace (under rocprofv3 --kernel-trace, on the GPU) or --summarise CSV")
