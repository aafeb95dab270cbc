#!/usr/bin/env python3
"""Times of the traceback on the tiled route (qecmc_class_minplus_tiled_chains) next to the sweep it traces, the sweep next to another
build of the library, and how often the traced correction is lighter than the default route's -> profiles/class_minplus_tiled_trace_rate.json.

    GPU box:  python3 tools/class_minplus_tiled_trace_rate.py [--out profiles/class_minplus_tiled_trace_rate.json] [--repeats 7] [--other-lib PATH]
              rocprofv3 --kernel-trace --stats -d DIR -o CASE --output-format csv -- python3 tools/class_minplus_tiled_trace_rate.py --one-call CASE
              python3 tools/class_minplus_tiled_trace_rate.py --kernels-from DIR      (folds the per-case kernel statistics into the JSON)

Per case -- rotated L = 13 at N = 256, rotated L = 21 at N = 4, planar L = 12 at N = 4, toric L = 7 at N = 1 -- qecmc_class_minplus_tiled_chains and
qecmc_class_minplus_tiled at unit costs on the same chains, in the same process, in ALTERNATING order: one warm call each, then `repeats` pairs.
Call time: between two device events on the null stream around one call (the representatives on the host, H2D, every launch, D2H): median, minimum
and maximum.  --other-lib: qecmc_class_minplus_tiled of this build and of the library at PATH (the parent commit's build) alternating in the same way:
its kernels are unchanged, so the two should differ by less than their spread.  Kernel times come from a rocprofv3 run of their own (--one-call runs
one warm and one measured traced call and nothing else).  Lighter: 64 syndromes at rotated L = 13, p = 0.1 through the harness, method min_weight on the
tiled route, with params['correction'] = "shortest_tiled" and without; the traced correction is never heavier (asserted).  No GPU: the tool fails."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = [("rotated", 13, 256), ("rotated", 21, 4), ("planar", 12, 4), ("toric", 7, 1)]
LIGHTER = ("rotated", 13, 64, 0.1)
KERNELS = {"k_class_minplus_tiled_trace": "trace", "k_class_minplus_tiled": "sweep", "k_minplus_pick": "pick", "k_minplus_tiled_walk": "walk",
           "k_class_minplus_reduce": "reduce"}
NOTE = ("call_ms: device events around one call (the representatives on the host and the copies included), qecmc_class_minplus_tiled_chains and "
        "qecmc_class_minplus_tiled at costs (0, 1, 1, 1) alternating on the same chains at the default widths; other_lib: qecmc_class_minplus_tiled of this build "
        "and of the parent commit's build alternating; kernel_ms: rocprofv3 --kernel-trace --stats of one traced call per case, a run of its own, the warm "
        "call's launches halved out; lighter: rows whose traced correction has fewer errors than qecmc.corrections' on the same syndromes")


def calls_of(lib, name, L, n):
    """(chains, minplus): the two calls of one case on the same chains, of the library `lib`"""
    from class_sweep_rate import CODES, random_chains
    from qecmc import _lib as L_
    code = CODES[name]
    flat = random_chains(name, L, n).reshape(n, -1)
    ncls = 16 if name == "toric" else 4
    costs = np.array([0, 1, 1, 1], np.uint32)
    cost, count, out = np.zeros((n, ncls), np.uint32), np.zeros((n, ncls), np.uint64), np.zeros((n, ncls, flat.shape[1]), np.uint8)
    keep = (flat, costs, cost, count, out)
    minplus = lambda: L_.check(lib.qecmc_class_minplus_tiled(code, L, n, L_.u8(flat), L_.u32(costs), 0, 0, L_.u32(cost), count.ctypes.data_as(L_._u64p), None))
    chains = None
    if hasattr(lib, "qecmc_class_minplus_tiled_chains"):
        chains = lambda: L_.check(lib.qecmc_class_minplus_tiled_chains(code, L, n, L_.u8(flat), L_.u32(costs), 0, 0, L_.u8(out), L_.u32(cost),
                                                                        count.ctypes.data_as(L_._u64p), None))
    return chains, minplus, keep


def event_ms(torch, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(torch, a_call, b_call, repeats):
    a_call(); b_call()                                                          # warm: code objects, pool blocks, the workspaces
    a, b = [], []
    for _ in range(repeats):
        a.append(event_ms(torch, a_call))
        b.append(event_ms(torch, b_call))
    return a, b


def stats(prefix, ms):
    return {prefix + "_ms_median": float(np.median(ms)), prefix + "_ms_min": float(min(ms)), prefix + "_ms_max": float(max(ms))}


def other_library(path):
    """the library at `path` with the argtypes of qecmc_class_minplus_tiled alone (a build that may lack the traced entry points)"""
    from qecmc import _lib as L_
    lib = C.CDLL(os.path.abspath(path))
    lib.qecmc_class_minplus_tiled.restype = C.c_int
    lib.qecmc_class_minplus_tiled.argtypes = L_.lib().qecmc_class_minplus_tiled.argtypes
    lib.qecmc_last_error.restype = C.c_char_p
    return lib


def measure(repeats, other):
    import torch
    import qecmc
    from qecmc import _lib as L_
    from qecmc.exact import sweep_tiled_info
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the times are measured on the device or not at all")
    torch.cuda.init()
    prop = torch.cuda.get_device_properties(0)
    rows = []
    for name, L, n in CASES:
        inf = sweep_tiled_info(name, L)
        chains, minplus, keep = calls_of(L_.lib(), name, L, n)
        a, b = alternate(torch, chains, minplus, repeats)
        row = dict(code=name, L=L, N=n, width=inf["width"], held=inf["held"], segments=inf["segments"], ncls=inf["ncls"])
        row.update(stats("chains_call", a)); row.update(stats("minplus_call", b))
        row.update(chains_over_minplus_call=row["chains_call_ms_median"] / row["minplus_call_ms_median"], larger_spread_ms=max(max(a) - min(a), max(b) - min(b)))
        if other:
            _, theirs, keep2 = calls_of(other_library(other), name, L, n)
            c, d = alternate(torch, minplus, theirs, repeats)
            row.update(stats("this_build_minplus_call", c)); row.update(stats("other_build_minplus_call", d))
            row.update(this_over_other=float(np.median(c)) / float(np.median(d)), other_larger_spread_ms=max(max(c) - min(c), max(d) - min(d)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows, dict(name=prop.name, compute_units=int(prop.multi_processor_count))


def lighter():
    from qecmc import harness
    name, L, n, p = LIGHTER
    params = dict(code=name, size=L, p_error=p, noise="depolarizing", method="min_weight", exact_method="tiled")
    default = harness.generate(params, n, seed=9, start="syndrome", corrections=True)
    traced = harness.generate(dict(params, correction="shortest_tiled"), n, seed=9, start="syndrome", corrections=True)
    assert np.array_equal(default["qubit_matrix"], traced["qubit_matrix"]) and np.array_equal(traced["success_correction"], traced["success"])
    assert np.all(traced["correction_weight"] <= default["correction_weight"]), "a traced correction is heavier than the default route's"
    diff = default["correction_weight"].astype(np.int64) - traced["correction_weight"].astype(np.int64)
    row = dict(code=name, L=L, N=n, p=p, lighter_rows=int((diff > 0).sum()), heavier_rows=int((diff < 0).sum()), largest_saving=int(diff.max()),
               mean_weight_traced=float(traced["correction_weight"].mean()), mean_weight_default=float(default["correction_weight"].mean()),
               success=int(traced["success"].sum()))
    print(json.dumps(row), flush=True)
    return row


def one_call(case):
    """one warm and one measured traced call of CASES[case], and nothing else: the program of a rocprofv3 run"""
    from qecmc import _lib as L_
    name, L, n = CASES[case]
    chains, _, keep = calls_of(L_.lib(), name, L, n)
    chains(); chains()


def fold_kernels(directory, out):
    """the kernel statistics rocprofv3 left per case (DIR/**/<case>_kernel_stats.csv) -> cases[i]['kernel_ms'] of the JSON at `out`: every launch ran twice
    (the warm call and the measured one), so totals and calls are halved"""
    res = json.load(open(out))
    for i, row in enumerate(res["cases"]):
        files = glob.glob(os.path.join(directory, "**", "%d_kernel_stats.csv" % i), recursive=True)
        if not files:
            continue
        kernel_ms = {}
        for r in csv.DictReader(open(files[0])):
            name = r.get("Name") or r.get("KernelName") or ""
            head = name.split("(")[0].split("::")[-1].strip()
            total = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
            key = KERNELS.get(head, KERNELS.get(head.replace("_site", ""), head))
            slot = kernel_ms.setdefault(key, dict(ms=0.0, launches=0))
            slot["ms"] += total / 2e6
            slot["launches"] += int(r.get("Calls") or 0) // 2
        row["kernel_ms"] = kernel_ms
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps([r.get("kernel_ms") for r in res["cases"]]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_minplus_tiled_trace_rate.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--one-call", type=int, default=None)
    ap.add_argument("--kernels-from", default=None)
    a = ap.parse_args()
    if a.one_call is not None:
        one_call(a.one_call)
    elif a.kernels_from:
        fold_kernels(a.kernels_from, a.out)
    else:
        if a.repeats < 5:
            sys.exit("--repeats: a median of at least 5")
        rows, dev = measure(a.repeats, a.other_lib)
        res = dict(device=dev, cases=rows, lighter=lighter(), note=NOTE)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
