#!/usr/bin/env python3
"""Times of the traceback (qecmc_class_minplus_chains) next to the sweep it traces -> profiles/class_minplus_trace_rate.json.

    GPU box:  python3 tools/class_minplus_trace_rate.py [--out profiles/class_minplus_trace_rate.json] [--repeats 9]
    GPU box:  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/class_minplus_trace_rate.py --trace
    anywhere: python3 tools/class_minplus_trace_rate.py --summarise OUT/<host>/<pid>_kernel_trace.csv [--out ...]
    GPU box:  rocprofv3 --kernel-trace --stats --output-format csv -d OUT_k -- python3 tools/class_minplus_trace_rate.py --trace-minplus SOME/libqecmc.so
    anywhere: python3 tools/class_minplus_trace_rate.py --summarise-ab this=OUT_1/..._kernel_trace.csv parent=OUT_2/... this=OUT_3/... parent=OUT_4/... [--out ...]

Per case -- rotated L = 9 at N = 1 024, toric L = 5 at N = 16, rotated L = 11 at N = 64, tools/class_minplus_rate.py's -- qecmc_class_minplus_chains and
qecmc_class_minplus at unit costs on the same chains, in the same process, in ALTERNATING order: one warm call each, then `repeats` pairs.
Call time: between two device events on the null stream around one call (the representatives on the host, H2D, every launch, D2H): median, minimum
and maximum.  Kernel time: the second form runs the same alternation (CALLS pairs per case) under a kernel trace, and the third adds up the
dispatches per kernel and call and merges the means into the JSON the first form wrote.  The fourth and fifth forms are the A/B of
qecmc_class_minplus alone, whose kernels this build does not change, against another build of the library (the parent commit's): alternating runs,
a process and a trace each, CALLS calls per case after a warm one; the summary keeps the mean of either build's run means and the larger spread of
the two series of runs.  No GPU: the measuring forms fail."""
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
CHAIN_KERNELS = ["sweep", "pick", "reduce", "trace", "walk"]                     # the dispatches of one qecmc_class_minplus_chains call of one launch group, in order
NOTE = ("call_ms: device events around one call (the representatives on the host and the copies included), qecmc_class_minplus_chains and qecmc_class_minplus "
        "at costs (0, 1, 1, 1) alternating on the same chains; *_kernel_us: rocprofv3 --kernel-trace, the dispatches of one call, mean of %d alternating calls "
        "in a run of its own; ab_*: the sweep and reduce kernels of qecmc_class_minplus alone, this build and the parent commit's in alternating runs of %d calls" % (CALLS, CALLS))


def calls_of(name, L, n, lib=None):
    """(chains, minplus): the two calls of one case on the same chains, and what they write"""
    from class_sweep_rate import CODES, random_chains
    from qecmc import _lib as L_
    lib, code = lib or L_.lib(), CODES[name]
    flat = random_chains(name, L, n).reshape(n, -1)
    ncls = 16 if name == "toric" else 4
    costs = np.array([0, 1, 1, 1], np.uint32)
    out = np.zeros((n, ncls, flat.shape[1]), np.uint8)
    cost, count = np.zeros((n, ncls), np.uint32), np.zeros((n, ncls), np.uint64)
    cost2, count2 = np.zeros((n, ncls), np.uint32), np.zeros((n, ncls), np.uint64)
    chains = lambda: L_.check(lib.qecmc_class_minplus_chains(code, L, n, L_.u8(flat), L_.u32(costs), 0, L_.u8(out), L_.u32(cost), count.ctypes.data_as(L_._u64p), None))
    minplus = lambda: L_.check(lib.qecmc_class_minplus(code, L, n, L_.u8(flat), L_.u32(costs), 0, L_.u32(cost2), count2.ctypes.data_as(L_._u64p), None))
    return chains, minplus, (out, cost, count, cost2, count2)


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
        chains, minplus, (out, cost, count, cost2, count2) = calls_of(name, L, n)
        chains(); minplus()                                                     # warm: code objects, pool blocks, the 128 KiB opt-ins
        assert np.array_equal(cost, cost2) and np.array_equal(count, count2) and np.all(count > 0) and out.max() <= 3
        a, b = [], []
        for _ in range(repeats):
            a.append(event_ms(torch, chains))
            b.append(event_ms(torch, minplus))
        med_a, med_b = float(np.median(a)), float(np.median(b))
        rows.append(dict(code=name, L=L, N=n, width=inf["width"], held=inf["held"], n_ops=inf["n_ops"], ncls=inf["ncls"],
                         workgroups_per_syndrome=inf["ncls"] << inf["held"], unique_share=float((count == 1).mean()),
                         chains_call_ms_median=med_a, chains_call_ms_min=float(min(a)), chains_call_ms_max=float(max(a)),
                         minplus_call_ms_median=med_b, minplus_call_ms_min=float(min(b)), minplus_call_ms_max=float(max(b)),
                         chains_over_minplus_call=med_a / med_b, larger_spread_ms=max(max(a) - min(a), max(b) - min(b))))
    return rows, dict(name=prop.name, compute_units=int(prop.multi_processor_count))


def trace():
    import qecmc
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible")
    for name, L, n in CASES:
        chains, minplus, _ = calls_of(name, L, n)
        chains(); minplus()
        for _ in range(CALLS):
            chains(); minplus()


def _mine(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows if "k_class_minplus" in r["Kernel_Name"] or "k_minplus_" in r["Kernel_Name"]]


def _load(out):
    return json.load(open(out)) if os.path.exists(out) else dict(cases=[dict(code=c, L=L, N=n) for c, L, n in CASES])


def summarise(path, out):
    mine = _mine(path)
    # every call of these cases is one launch group: five dispatches of the traceback, two of the sweep; per case a warm pair of calls, then CALLS pairs
    per_pair = len(CHAIN_KERNELS) + 2
    per_case = per_pair * (CALLS + 1)
    assert len(mine) == per_case * len(CASES), (len(mine), per_case)
    res = _load(out)
    for k, (name, L, n) in enumerate(CASES):
        timed = mine[k * per_case + per_pair:(k + 1) * per_case]                # (the warm pair left out)
        us = {}
        for i, (kernel, ns) in enumerate(timed):
            pos = i % per_pair
            key = "chains_" + CHAIN_KERNELS[pos] if pos < len(CHAIN_KERNELS) else "minplus_" + ("sweep", "reduce")[pos - len(CHAIN_KERNELS)]
            want = {"sweep": "k_class_minplus", "reduce": "k_class_minplus_reduce", "pick": "k_minplus_pick", "trace": "k_minplus_trace", "walk": "k_minplus_walk"}[key.split("_")[1]]
            assert want in kernel and (want != "k_class_minplus" or "reduce" not in kernel), (i, key, kernel)
            us[key] = us.get(key, 0.0) + ns / 1e3 / CALLS
        row = next(r for r in res["cases"] if (r["code"], r["L"], r["N"]) == (name, L, n))
        row.update({"%s_kernel_us" % key: v for key, v in sorted(us.items())})
        extra = us["chains_pick"] + us["chains_trace"] + us["chains_walk"]
        row["traceback_extra_kernel_us"] = extra
        row["traceback_extra_over_sweep_kernel"] = extra / (us["minplus_sweep"] + us["minplus_reduce"])
        print(json.dumps(row))
    res["note"] = NOTE
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def trace_minplus(path):
    """qecmc_class_minplus alone, from the library at `path` (bound by hand: a parent build lacks this build's newer entry points)"""
    from qecmc import _lib as L_
    lib = C.CDLL(os.path.abspath(path))
    for name in ("qecmc_class_minplus", "qecmc_device_count"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L_.SIGNATURES[name]
    if lib.qecmc_device_count() < 1:
        sys.exit("no GPU visible")
    for name, L, n in CASES:
        _, minplus, (_, _, _, cost, count) = calls_of(name, L, n, lib=lib)
        minplus()
        assert np.all(count > 0)
        for _ in range(CALLS):
            minplus()


def summarise_ab(runs, out):
    """runs: "this=CSV" and "parent=CSV", the kernel traces of alternating --trace-minplus runs of the two builds"""
    per_case = 2 * (CALLS + 1)                                                  # (sweep, reduce) per call; a warm call, then CALLS
    means = {"this": [[] for _ in CASES], "parent": [[] for _ in CASES]}
    for run in runs:
        label, path = run.split("=", 1)
        mine = [m for m in _mine(path) if "k_class_minplus" in m[0]]
        assert len(mine) == per_case * len(CASES), (run, len(mine), per_case)
        for k in range(len(CASES)):
            timed = mine[k * per_case + 2:(k + 1) * per_case]
            means[label][k].append(sum(ns for _, ns in timed) / 1e3 / CALLS)
    res = _load(out)
    for k, (name, L, n) in enumerate(CASES):
        new, old = means["this"][k], means["parent"][k]
        row = next(r for r in res["cases"] if (r["code"], r["L"], r["N"]) == (name, L, n))
        row.update(ab_minplus_kernel_us_this_build=float(np.mean(new)), ab_minplus_kernel_us_parent=float(np.mean(old)), ab_runs_each=len(new),
                   ab_difference_us=float(np.mean(new) - np.mean(old)), ab_larger_spread_us=float(max(max(new) - min(new), max(old) - min(old))))
        row["ab_within_spread"] = bool(abs(row["ab_difference_us"]) <= row["ab_larger_spread_us"])
        print(json.dumps(row))
    res["note"] = NOTE
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_minplus_trace_rate.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="run the alternating calls alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--summarise", default=None, help="a kernel_trace.csv written by rocprofv3 around a --trace run: merge the kernel times into --out")
    ap.add_argument("--trace-minplus", default=None, metavar="LIBQECMC", help="run qecmc_class_minplus alone from that build of the library, for rocprofv3 --kernel-trace")
    ap.add_argument("--summarise-ab", default=None, nargs="+", metavar="this=CSV|parent=CSV",
                    help="the kernel traces of alternating --trace-minplus runs of this build and the parent's: merge both means and the larger spread into --out")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out)
    elif a.summarise_ab:
        summarise_ab(a.summarise_ab, a.out)
    elif a.trace_minplus:
        trace_minplus(a.trace_minplus)
    elif a.trace:
        trace()
    else:
        rows, dev = measure(a.repeats)
        res = dict(device=dev, cases=rows, note=NOTE)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
