#!/usr/bin/env python3
"""Rates of the frontier sweep (qecmc_class_sweep) -> profiles/class_sweep_rate.json.

    GPU box:  python3 tools/class_sweep_rate.py [--out profiles/class_sweep_rate.json] [--repeats 7]

Per case -- xzzx L = 5 with N = 64 (the one shape both methods take: the enumerator is timed in the same process, right after), xzzx L = 7 and
rotated L = 9 with N = 1 024, planar L = 6 with N = 256, toric L = 3 with N = 4 096 -- the time of one warm call between two device events on the
null stream (the representatives on the host, H2D, every launch, D2H), median and spread of `repeats`; the class-LDS-updates of the call (one update:
one entry of the state vector read, changed and written by one op, counted from the op stream: 2^(occupied slots) per op, per class, per syndrome)
per second from the median; and the share of the LDS bandwidth bound: ops x 2^width x 16 bytes per class against 256 bytes per clock and CU (the
width of the LDS array) at the peak engine clock.  No GPU: the script fails."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
CSRC = os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc")
CASES = [("xzzx", 5, 64), ("xzzx", 7, 1024), ("rotated", 9, 1024), ("planar", 6, 256), ("toric", 3, 4096)]
CODES = {"toric": 0, "xzzx": 1, "rotated": 2, "planar": 3}
LDS_BYTES_PER_CLOCK_AND_CU = 256.0


def random_chains(code, L, n, seed=0):
    rng = np.random.default_rng([19, L, n, seed])
    shape = (n, 2, L, L) if code in ("toric", "planar") else (n, L, L)
    m = np.zeros(shape, dtype=np.uint8)
    err = rng.random(shape) < 0.15
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    if code == "planar":
        m[:, 1, -1, :] = 0
        m[:, 1, :, -1] = 0
    return m


def updates_per_class(code, L, n_ops):
    """live entries summed over the op stream, from the host-table test library"""
    subprocess.check_call(["make", "-C", CSRC, "-s", "tables"])
    T = C.CDLL(os.path.join(CSRC, "build", "libqecmc_tables.so"))
    buf = np.zeros(4 * n_ops, np.uint32)
    T.qt_class_sweep_ops.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int]
    assert T.qt_class_sweep_ops(CODES[code], L, buf.ctypes.data, buf.size) == buf.size
    return int(sum(1 << bin(mask).count("1") for mask in buf.reshape(-1, 4)[:, 1].tolist()))


def events(torch, call, repeats):
    """ms between two device events around one call, after a warm-up: [repeats]"""
    call()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def gpu_cases(repeats, peak_mhz):
    import torch
    import qecmc
    from qecmc import _lib as L_
    from qecmc.exact import depolarizing_w4, enumerator_info, sweep_info
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the rates are measured on the device or not at all")
    lib = L_.lib()
    torch.cuda.init()
    prop = torch.cuda.get_device_properties(0)
    cus = int(prop.multi_processor_count)
    f64p = C.POINTER(C.c_double)
    w = depolarizing_w4(0.1)
    rows = []
    for name, L, n in CASES:
        code, inf = CODES[name], sweep_info(name, L)
        flat = random_chains(name, L, n).reshape(n, -1)
        z = np.zeros((n, inf["ncls"]))
        ms = events(torch, lambda: L_.check(lib.qecmc_class_sweep(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), z.ctypes.data_as(f64p), None)), repeats)
        assert np.all(z > 0)
        med = float(np.median(ms))
        updates = n * inf["ncls"] * updates_per_class(name, L, inf["n_ops"])
        bound_s = n * inf["ncls"] * inf["n_ops"] * (1 << inf["width"]) * 16.0 / (LDS_BYTES_PER_CLOCK_AND_CU * cus * peak_mhz * 1e6)
        row = dict(code=name, L=L, N=n, width=inf["width"], n_ops=inf["n_ops"], ncls=inf["ncls"], call_ms_median=med, call_ms_min=float(min(ms)),
                   call_ms_max=float(max(ms)), class_lds_updates=updates, class_lds_updates_per_s_of_the_call=updates / (med * 1e-3),
                   lds_bound_ms=bound_s * 1e3, share_of_the_lds_bound=bound_s * 1e3 / med)
        if (name, L) == ("xzzx", 5):                                            # the same chains through the enumerator, in the same visit
            e = enumerator_info(name, L)
            hist = np.zeros((n, e["ncls"], e["nq"] + 1, e["nq"] + 1), dtype=np.uint64)
            em = events(torch, lambda: L_.check(lib.qecmc_coset_enumerate(code, L, n, L_.u8(flat), 0, 0, 0, hist.ctypes.data_as(L_._u64p), None)), repeats)
            k = np.arange(e["nq"] + 1, dtype=np.float64)
            want = np.einsum("scij,ij->sc", hist.astype(np.float64), w[1] ** (k[:, None] + k[None, :]))
            assert (np.abs(z - want) / want).max() < 1e-12
            row.update(enumerator_call_ms_median=float(np.median(em)), enumerator_call_ms_min=float(min(em)), enumerator_call_ms_max=float(max(em)),
                       sweep_over_enumerator=med / float(np.median(em)))
        rows.append(row)
    return rows, dict(name=prop.name, compute_units=cus, peak_clock_mhz=peak_mhz)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_sweep_rate.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--peak-clock-mhz", type=float, default=2400.0, help="the peak engine clock the LDS bound is stated at (MI355X: 2400)")
    a = ap.parse_args()
    rows, dev = gpu_cases(a.repeats, a.peak_clock_mhz)
    res = dict(device=dev, cases=rows,
               note="call_ms: device events around one qecmc_class_sweep call (the representatives on the host and the copies included); "
                    "lds_bound_ms: N x ncls x n_ops x 2^width x 16 bytes at 256 bytes per clock and CU -- an op that walks fewer than 2^width entries "
                    "makes the call faster than the figure suggests")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
