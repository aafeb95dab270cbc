#!/usr/bin/env python3
"""Rates of the cut-set sweep (qecmc_class_sweep_cut) -> profiles/class_sweep_cut_rate.json.

    GPU box:  python3 tools/class_sweep_cut_rate.py [--out profiles/class_sweep_cut_rate.json] [--repeats 7]

Per case the time of one warm call between two device events on the null stream (the representatives on the host, H2D, every launch, D2H): median,
minimum and maximum of `repeats`.  Toric L = 5 at N = 1 and 16 under lds_width 13 (8 held, two workgroups per CU) and 14 (7 held, one per CU): the
default width of that shape is the faster of the two.  xzzx L = 11, rotated L = 11 and planar L = 7 at N = 64 through the 128 KiB state vector.
Rotated L = 9 (width 12) and toric L = 3 (width 13) at N = 1 024 with nothing held against qecmc_class_sweep on the same chains in the same process:
the two do the same work, and the results are compared bit for bit.  No GPU: the script fails."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from class_sweep_rate import CODES, events, random_chains  # noqa: E402

CASES = [("toric", 5, 1, 13), ("toric", 5, 1, 14), ("toric", 5, 16, 13), ("toric", 5, 16, 14), ("xzzx", 11, 64, 0), ("rotated", 11, 64, 0),
         ("planar", 7, 64, 0), ("rotated", 9, 1024, 0), ("toric", 3, 1024, 0)]


def gpu_cases(repeats):
    import torch
    import qecmc
    from qecmc import _lib as L_
    from qecmc.exact import depolarizing_w4, sweep_cut_info
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the rates are measured on the device or not at all")
    lib = L_.lib()
    torch.cuda.init()
    prop = torch.cuda.get_device_properties(0)
    f64p = C.POINTER(C.c_double)
    w = depolarizing_w4(0.1)
    rows = []
    for name, L, n, lds_width in CASES:
        code, inf = CODES[name], sweep_cut_info(name, L, lds_width)
        flat = random_chains(name, L, n).reshape(n, -1)
        z = np.zeros((n, inf["ncls"]))
        ms = events(torch, lambda: L_.check(lib.qecmc_class_sweep_cut(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), lds_width, z.ctypes.data_as(f64p), None)), repeats)
        assert np.all(z > 0)
        med = float(np.median(ms))
        row = dict(code=name, L=L, N=n, lds_width=lds_width, full_width=inf["full_width"], width=inf["width"], held=inf["held"], n_ops=inf["n_ops"],
                   ncls=inf["ncls"], workgroups_per_syndrome=inf["ncls"] << inf["held"], call_ms_median=med, call_ms_min=float(min(ms)),
                   call_ms_max=float(max(ms)), ms_per_syndrome=med / n)
        if inf["held"] == 0 and inf["width"] <= 13:                             # the same chains through qecmc_class_sweep, in the same visit
            z0 = np.zeros_like(z)
            m0 = events(torch, lambda: L_.check(lib.qecmc_class_sweep(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), z0.ctypes.data_as(f64p), None)), repeats)
            assert np.array_equal(z.view(np.uint64), z0.view(np.uint64))
            spread = max(max(ms) - min(ms), max(m0) - min(m0))
            row.update(uncut_call_ms_median=float(np.median(m0)), uncut_call_ms_min=float(min(m0)), uncut_call_ms_max=float(max(m0)),
                       cut_minus_uncut_ms=med - float(np.median(m0)), larger_spread_ms=spread,
                       slower_by_more_than_three_spreads=bool(med - float(np.median(m0)) > 3 * spread))
        rows.append(row)
    return rows, dict(name=prop.name, compute_units=int(prop.multi_processor_count))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_sweep_cut_rate.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--library", default=None, help="another build of libqecmc.so (e.g. one made with -DQECMC_CUT_THREADS_W14=512) instead of the in-tree one")
    ap.add_argument("--label", default="in-tree build", help="what the build is, for the record")
    a = ap.parse_args()
    if a.library:
        from qecmc import _lib
        _lib.use_library(a.library)
    rows, dev = gpu_cases(a.repeats)
    res = dict(device=dev, build=a.label, cases=rows,
               note="call_ms: device events around one qecmc_class_sweep_cut call (the representatives on the host and the copies included); "
                    "uncut_*: qecmc_class_sweep on the same chains in the same process")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
