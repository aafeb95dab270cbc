#!/usr/bin/env python3
"""Times of the (min, +, count) sweep (qecmc_class_minplus) next to its double sibling -> profiles/class_minplus_rate.json.

    GPU box:  python3 tools/class_minplus_rate.py [--out profiles/class_minplus_rate.json] [--repeats 9]
    GPU box:  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/class_minplus_rate.py --trace
    anywhere: python3 tools/class_minplus_rate.py --summarise OUT/<host>/<pid>_kernel_trace.csv [--out profiles/class_minplus_rate.json]

Per case -- rotated L = 9 at N = 1 024, toric L = 5 at N = 16, rotated L = 11 at N = 64 -- qecmc_class_minplus at unit costs and qecmc_class_sweep_cut
at depolarizing weights on the same chains, in the same process, in ALTERNATING order: one warm call each, then `repeats` pairs.
Call time: between two device events on the null stream around one call (the representatives on the host, H2D, every launch, D2H): median, minimum
and maximum.  Kernel time: the second form runs the same alternation (CALLS pairs per case) under a kernel trace, and the third adds up the
dispatches of each entry point's two kernels per call and merges the means into the JSON the first form wrote.  No GPU: the first two forms fail."""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = [("rotated", 9, 1024), ("toric", 5, 16), ("rotated", 11, 64)]
CALLS = 5
NOTE = ("call_ms: device events around one call (the representatives on the host and the copies included), qecmc_class_minplus at costs (0, 1, 1, 1) and "
        "qecmc_class_sweep_cut at depolarizing_w4(0.1) alternating on the same chains; kernel_us: rocprofv3 --kernel-trace, the sweep kernel's and the reduce "
        "kernel's dispatches of one call, mean of %d alternating calls in a run of its own" % CALLS)


def calls_of(name, L, n):
    """(minplus, cut): the two calls of one case on the same chains, and what they write"""
    from class_sweep_rate import CODES, random_chains
    from qecmc import _lib as L_
    from qecmc.exact import depolarizing_w4
    lib, code = L_.lib(), CODES[name]
    flat = random_chains(name, L, n).reshape(n, -1)
    ncls = 16 if name == "toric" else 4
    costs, w = np.array([0, 1, 1, 1], np.uint32), depolarizing_w4(0.1)
    cost, count, z = np.zeros((n, ncls), np.uint32), np.zeros((n, ncls), np.uint64), np.zeros((n, ncls))
    f64p = C.POINTER(C.c_double)
    minplus = lambda: L_.check(lib.qecmc_class_minplus(code, L, n, L_.u8(flat), L_.u32(costs), 0, L_.u32(cost), count.ctypes.data_as(L_._u64p), None))
    cut = lambda: L_.check(lib.qecmc_class_sweep_cut(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), 0, z.ctypes.data_as(f64p), None))
    return minplus, cut, (cost, count, z)


def event_ms(torch, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(repeats):
    import torch
    import qecmc
    from qecmc.exact import sweep_cut_info
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the times are measured on the device or not at all")
    torch.cuda.init()
    prop = torch.cuda.get_device_properties(0)
    rows = []
    for name, L, n in CASES:
        inf = sweep_cut_info(name, L, 0)
        minplus, cut, (cost, count, z) = calls_of(name, L, n)
        minplus(); cut()                                                        # warm: code objects, pool blocks, the 128 KiB opt-ins
        assert np.all(count > 0) and np.all(z > 0)
        a, b = [], []
        for _ in range(repeats):
            a.append(event_ms(torch, minplus))
            b.append(event_ms(torch, cut))
        med_a, med_b = float(np.median(a)), float(np.median(b))
        spread = max(max(a) - min(a), max(b) - min(b))
        rows.append(dict(code=name, L=L, N=n, width=inf["width"], held=inf["held"], n_ops=inf["n_ops"], ncls=inf["ncls"],
                         workgroups_per_syndrome=inf["ncls"] << inf["held"], largest_count=int(count.max()), largest_cost=int(cost.max()),
                         minplus_call_ms_median=med_a, minplus_call_ms_min=float(min(a)), minplus_call_ms_max=float(max(a)),
                         cut_call_ms_median=med_b, cut_call_ms_min=float(min(b)), cut_call_ms_max=float(max(b)),
                         minplus_over_cut_call=med_a / med_b, larger_spread_ms=spread))
    return rows, dict(name=prop.name, compute_units=int(prop.multi_processor_count))


def trace():
    import qecmc
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible")
    for name, L, n in CASES:
        minplus, cut, _ = calls_of(name, L, n)
        minplus(); cut()
        for _ in range(CALLS):
            minplus(); cut()


def summarise(path, out):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    mine = [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows
            if "k_class_minplus" in r["Kernel_Name"] or "k_class_sweep_cut" in r["Kernel_Name"] or "k_class_sweep_reduce" in r["Kernel_Name"]]
    # every call of these cases is one launch group: a sweep kernel and a reduce kernel; per case a warm pair of calls, then CALLS pairs
    per_case = 2 * 2 * (CALLS + 1)
    assert len(mine) == per_case * len(CASES), (len(mine), per_case)
    res = json.load(open(out)) if os.path.exists(out) else dict(cases=[dict(code=c, L=L, N=n) for c, L, n in CASES])
    for k, (name, L, n) in enumerate(CASES):
        timed = mine[k * per_case + 4:(k + 1) * per_case]                       # (the warm pair left out)
        us = {}
        for kernel, ns in timed:
            key = "minplus_sweep" if "k_class_minplus_reduce" not in kernel and "k_class_minplus" in kernel else "minplus_reduce" if "k_class_minplus_reduce" in kernel \
                else "cut_sweep" if "k_class_sweep_cut" in kernel else "cut_reduce"
            us[key] = us.get(key, 0.0) + ns / 1e3 / CALLS
        row = next(r for r in res["cases"] if (r["code"], r["L"], r["N"]) == (name, L, n))
        row.update({"%s_kernel_us" % key: v for key, v in sorted(us.items())})
        row["minplus_over_cut_kernel"] = (us["minplus_sweep"] + us["minplus_reduce"]) / (us["cut_sweep"] + us["cut_reduce"])
        print(json.dumps(row))
    res["note"] = NOTE
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_minplus_rate.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="run the alternating calls alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--summarise", default=None, help="a kernel_trace.csv written by rocprofv3 around a --trace run: merge the kernel times into --out")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out)
    elif a.trace:
        trace()
    else:
        rows, dev = measure(a.repeats)
        res = dict(device=dev, cases=rows, note=NOTE)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
