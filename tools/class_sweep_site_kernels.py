#!/usr/bin/env python3
"""Kernel time alone of the site sweeps against their siblings -> profiles/class_sweep_site_kernel_trace.json.

    GPU box:  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/class_sweep_site_kernels.py
    anywhere: python3 tools/class_sweep_site_kernels.py --summarise OUT/<host>/<pid>_kernel_trace.csv [--out profiles/class_sweep_site_kernel_trace.json]

tools/class_sweep_site_rate.py times whole calls, host work included.  This one separates the kernels: per shape five calls of the uniform entry
point, five of the site route with one table and five with one table per syndrome, in that order, under a kernel trace; the summary adds up the
dispatches of every call (the sweep kernel's launches and the reduce; the runtime's copy kernels are left out) and reports the mean per call."""
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

# (route, code, L, N, widths)
CASES = [("sweep", "xzzx", 7, 1024, ()), ("sweep", "rotated", 9, 1024, ()), ("sweep", "toric", 3, 4096, ()), ("cut", "rotated", 11, 64, (0,)),
         ("cut", "toric", 5, 16, (13,)), ("tiled", "rotated", 13, 256, (0, 0)), ("tiled", "rotated", 21, 1, (0, 0))]
CALLS = 5


def run():
    from class_sweep_rate import CODES, random_chains
    import qecmc
    from qecmc import _lib as L_
    from qecmc.exact import depolarizing_site_w4, depolarizing_w4
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible")
    lib = L_.lib()
    f64p = C.POINTER(C.c_double)
    w = depolarizing_w4(0.1)
    for route, name, L, n, widths in CASES:
        code = CODES[name]
        flat = random_chains(name, L, n).reshape(n, -1)
        nq = flat.shape[1]
        one = np.ascontiguousarray(np.broadcast_to(w, (1, nq, 4)))
        per = depolarizing_site_w4(np.random.default_rng([23, L, n]).uniform(0.05, 0.15, size=(n, nq)))
        z = np.zeros((n, 16 if name == "toric" else 4))
        uniform = {"sweep": lib.qecmc_class_sweep, "cut": lib.qecmc_class_sweep_cut, "tiled": lib.qecmc_class_sweep_tiled}[route]
        site = {"sweep": lib.qecmc_class_sweep_site, "cut": lib.qecmc_class_sweep_cut_site, "tiled": lib.qecmc_class_sweep_tiled_site}[route]
        for _ in range(CALLS):
            L_.check(uniform(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), *widths, z.ctypes.data_as(f64p), None))
        for _ in range(CALLS):
            L_.check(site(code, L, n, L_.u8(flat), one.ctypes.data_as(f64p), 1, *widths, z.ctypes.data_as(f64p), None))
        for _ in range(CALLS):
            L_.check(site(code, L, n, L_.u8(flat), per.ctypes.data_as(f64p), n, *widths, z.ctypes.data_as(f64p), None))


def summarise(path, out):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ns = [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows if "k_class_sweep" in r["Kernel_Name"]]
    # the dispatches of one shape: 5 uniform calls, then 10 site calls; all calls of a shape launch the same number of kernels
    res, i = [], 0
    for route, name, L, n, widths in CASES:
        j = i
        while j < len(ns) and ("_site" not in ns[j][0]):
            j += 1
        per_call = (j - i) // CALLS
        assert per_call >= 1 and (j - i) == per_call * CALLS, (route, name, L, j - i)
        phases = [sum(d for _, d in ns[i + k * per_call * CALLS:i + (k + 1) * per_call * CALLS]) / CALLS / 1e3 for k in range(3)]
        i += 3 * per_call * CALLS
        res.append(dict(route=route, code=name, L=L, N=n, widths=list(widths), kernels_per_call=per_call, uniform_kernel_us_per_call=phases[0],
                        site_one_table_kernel_us_per_call=phases[1], site_per_syndrome_kernel_us_per_call=phases[2],
                        one_table_over_uniform=phases[1] / phases[0], per_syndrome_over_uniform=phases[2] / phases[0]))
    assert i == len(ns), (i, len(ns))
    with open(out, "w") as f:
        json.dump(dict(cases=res, note="kernel time from rocprofv3 --kernel-trace, mean of 5 calls each: the sweep kernel's dispatches and the reduce of a call"), f, indent=1)
    for r in res:
        print(json.dumps(r))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", default=None, help="a kernel_trace.csv written by rocprofv3 around a run of this script")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_sweep_site_kernel_trace.json"))
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out)
    else:
        run()
