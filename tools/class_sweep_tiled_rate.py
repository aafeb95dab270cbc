#!/usr/bin/env python3
"""Rates of the sweep tiled over HBM (qecmc_class_sweep_tiled) -> profiles/class_sweep_tiled_rate.json.

    GPU box:  python3 tools/class_sweep_tiled_rate.py [--out profiles/class_sweep_tiled_rate.json] [--repeats 7] [--only toric7,tile,calls,small]

Per case the time of one warm call between two device events on the null stream (the representatives on the host, H2D, every launch, D2H): median,
minimum and maximum of `repeats`.  Four groups:
  toric7  the toric code at L = 7, one syndrome, under hbm_width 24, 22 and 20 (5, 7 and 9 held): the default hbm_width is the fastest;
  tile    rotated L = 17 (8 syndromes) and L = 21 (one) under tile_width 13, 12, 11 and 10, rotated L = 13 (256) and toric L = 7 (one) under 13 and
          11: the default tile_width likewise;
  calls   rotated L = 13, 17, 21 and planar L = 12 at the defaults, against two bounds counted from the plan itself -- the LDS bound of DESIGN.md 4.1k
          (live entries walked x 16 bytes at 256 bytes per clock and CU) and the HBM bytes of the segment table at the 8 TB/s of the data sheet;
  small   toric L = 3 and rotated L = 9 at N = 1 024 against qecmc_class_sweep on the same chains in the same process, bit for bit: what the extra
          launches cost where nothing routes by default.
The counts come from the host-table test library (csrc: make tables), which holds the planner.  No GPU: the script fails."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from class_sweep_rate import CODES, events, random_chains  # noqa: E402

# (group, code, L, N, hbm_width, tile_width)
CASES = [("toric7", "toric", 7, 1, 24, 0), ("toric7", "toric", 7, 1, 22, 0), ("toric7", "toric", 7, 1, 20, 0),
         ("tile", "rotated", 17, 8, 0, 13), ("tile", "rotated", 17, 8, 0, 12), ("tile", "rotated", 17, 8, 0, 11), ("tile", "rotated", 17, 8, 0, 10),
         ("tile", "rotated", 21, 1, 0, 13), ("tile", "rotated", 21, 1, 0, 12), ("tile", "rotated", 21, 1, 0, 11), ("tile", "rotated", 21, 1, 0, 10),
         ("tile", "rotated", 13, 256, 0, 13), ("tile", "rotated", 13, 256, 0, 11), ("tile", "toric", 7, 1, 24, 13), ("tile", "toric", 7, 1, 24, 11),
         ("calls", "rotated", 13, 256, 0, 0), ("calls", "rotated", 17, 16, 0, 0), ("calls", "rotated", 21, 1, 0, 0), ("calls", "rotated", 21, 2, 0, 0),
         ("calls", "planar", 12, 1, 0, 0),
         ("small", "toric", 3, 1024, 0, 0), ("small", "rotated", 9, 1024, 0, 0)]
HBM_BYTES_PER_S = 8.0e12
_u32p = C.POINTER(C.c_uint32)


def plan_counts(code, L, hbm_width, tile_width, n_ops, n_segments):
    """per (class, assignment): the live entries the ops walk, and the entries gathered from and stored to HBM, from the planner's own tables"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "tables"])
    lib = C.CDLL(os.path.join(CSRC, "build", "libqecmc_tables.so"))
    ops, segs = np.zeros(4 * n_ops, np.uint32), np.zeros(8 * n_segments, np.uint32)
    assert lib.qt_class_sweep_tiled_ops(code, L, hbm_width, tile_width, ops.ctypes.data_as(_u32p), ops.size) == ops.size
    assert lib.qt_class_sweep_tiled_segments(code, L, hbm_width, tile_width, segs.ctypes.data_as(_u32p), segs.size) == segs.size
    pop = lambda v: bin(int(v)).count("1")
    entry_ops = sum(1 << pop(m) for m in ops.reshape(-1, 4)[:, 1])
    segs = segs.reshape(-1, 8)
    moved = sum(1 << pop(s[4]) for s in segs[1:]) + sum(1 << pop(s[5]) for s in segs[:-1])
    return entry_ops, moved, int(max(s[6] for s in segs))


def gpu_cases(repeats, only, peak_mhz):
    import torch
    import qecmc
    from qecmc import _lib as L_
    from qecmc.exact import depolarizing_w4, sweep_tiled_info
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the rates are measured on the device or not at all")
    lib = L_.lib()
    torch.cuda.init()
    prop = torch.cuda.get_device_properties(0)
    cus = int(prop.multi_processor_count)
    f64p = C.POINTER(C.c_double)
    w = depolarizing_w4(0.1)
    rows = []
    for group, name, L, n, hbm_width, tile_width in CASES:
        if group not in only:
            continue
        code, inf = CODES[name], sweep_tiled_info(name, L, hbm_width, tile_width)
        flat = random_chains(name, L, n).reshape(n, -1)
        z = np.zeros((n, inf["ncls"]))
        ms = events(torch, lambda: L_.check(lib.qecmc_class_sweep_tiled(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), hbm_width, tile_width,
                                                                         z.ctypes.data_as(f64p), None)), repeats)
        assert np.all(z > 0)
        med = float(np.median(ms))
        entry_ops, moved, tiles = plan_counts(code, L, hbm_width, tile_width, inf["n_ops"], inf["segments"])
        units = n * inf["ncls"] << inf["held"]
        lds_bound = units * entry_ops * 16 / (256.0 * cus * peak_mhz * 1e6) * 1e3
        hbm_bound = units * moved * 8 / HBM_BYTES_PER_S * 1e3
        row = dict(group=group, code=name, L=L, N=n, hbm_width=hbm_width, tile_width=tile_width, full_width=inf["full_width"], width=inf["width"],
                   held=inf["held"], n_ops=inf["n_ops"], segments=inf["segments"], ncls=inf["ncls"], units=units, most_tiles_of_a_segment=tiles,
                   call_ms_median=med, call_ms_min=float(min(ms)), call_ms_max=float(max(ms)), ms_per_syndrome=med / n,
                   entry_ops_per_unit=entry_ops, entry_ops_per_s_of_the_call=units * entry_ops / (med * 1e-3), lds_bound_ms=lds_bound,
                   hbm_entries_per_unit=moved, hbm_bytes_of_the_call=units * moved * 8, hbm_bytes_per_s_of_the_call=units * moved * 8 / (med * 1e-3),
                   hbm_bound_ms=hbm_bound, call_over_the_larger_bound=med / max(lds_bound, hbm_bound))
        if group == "small":                                                    # the same chains through qecmc_class_sweep, in the same visit
            z0 = np.zeros_like(z)
            m0 = events(torch, lambda: L_.check(lib.qecmc_class_sweep(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), z0.ctypes.data_as(f64p), None)), repeats)
            assert np.array_equal(z.view(np.uint64), z0.view(np.uint64))
            row.update(lds_sweep_call_ms_median=float(np.median(m0)), lds_sweep_call_ms_min=float(min(m0)), lds_sweep_call_ms_max=float(max(m0)),
                       tiled_over_lds_sweep=med / float(np.median(m0)))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows, dict(name=prop.name, compute_units=cus, peak_clock_mhz=peak_mhz)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_sweep_tiled_rate.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", default="toric7,tile,calls,small")
    ap.add_argument("--peak-mhz", type=float, default=2400.0)
    a = ap.parse_args()
    rows, dev = gpu_cases(a.repeats, a.only.split(","), a.peak_mhz)
    res = dict(device=dev, cases=rows,
               note="call_ms: device events around one qecmc_class_sweep_tiled call (the representatives on the host and the copies included); units: "
                    "N x ncls x 2^held state vectors; lds_bound_ms: units x live entries walked x 16 bytes at 256 bytes per clock and CU; hbm_bound_ms: "
                    "units x entries gathered and stored x 8 bytes at 8 TB/s; lds_sweep_*: qecmc_class_sweep on the same chains in the same process")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
