#!/usr/bin/env python3
"""Times of the exact sampler on the tiled route (qecmc_class_sample_tiled) next to the sweep it records, the bytes both move, the walk
per sample, the sweep next to another build of the library, one call past the default cap, and the purpose row: rung 0 of the samplers against exact
draws at rotated L = 13 -> profiles/class_sample_tiled_rate.json.

    GPU box:  python3 tools/class_sample_tiled_rate.py [--out profiles/class_sample_tiled_rate.json] [--repeats 7] [--other-lib PATH] [--skip-l21]

Per case -- rotated L = 13 at N = 16, L = 15 at N = 4, L = 17 at N = 1 -- qecmc_class_sample_tiled (every-class mode, depolarizing p = 0.1, K = 1) and
qecmc_class_sweep_tiled on the same chains, in the same process, in ALTERNATING order: one warm call each, then `repeats` pairs.  Call time: between
two device events on the null stream around one call (the representatives on the host, H2D, every launch, D2H): median, minimum and maximum.  With
nothing held a sampler call sweeps every (syndrome, class) pair once for the partials and once more for the record, so the expected ratio of the two
calls is 1 + (state bytes + record bytes) / state bytes, the bytes counted from the segment table: a segment gathers the entries live at its first op
and stores those live after its last, 8 bytes each, and a FORGET stores 16 bytes per live pair slot of every live tile (bytes_per_job).  The walk:
calls at K = 64 and K = 1 024 against K = 1, per sample beyond the first.  --other-lib: qecmc_class_sweep_tiled of this build and of the library at PATH
(the parent commit's build) alternating in the same way: the kernels are the same, so the two should differ by less than their spread.  L = 21: one
posterior call, N = 1, K = 1, record_bytes = 40 GiB, if the card has 48 GiB free.  Purpose: 32 syndromes at rotated L = 13, p = 0.1; rung 0's mean
error count over 20 000 ladder steps after 2 000 (scan = random and scan = wave) against 1 024 exact draws per syndrome, paired by syndrome, in
error bars std(d) / sqrt(32): written down, not gated.  No GPU: the tool fails."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = [("rotated", 13, 16), ("rotated", 15, 4), ("rotated", 17, 1)]
KS = (64, 1024)
P = 0.1
PURPOSE = ("rotated", 13, 32, 20000, 2000)
NOTE = ("call_ms: device events around one call (the representatives on the host and the copies included), qecmc_class_sample_tiled (mode 0, K = 1) and "
        "qecmc_class_sweep_tiled at depolarizing p = 0.1 alternating on the same chains at the default widths; byte_ratio = (state + record) / state bytes of one "
        "unit from the segment table, expected_call_ratio = 1 + byte_ratio; walk_us_per_sample: (call at K - call at 1) / ((K - 1) * N * ncls); other_lib: "
        "qecmc_class_sweep_tiled of this build and of the parent commit's build alternating; purpose: d = rung 0's mean error count - the mean of 1 024 exact "
        "draws, per syndrome")


def segment_bytes(name, L):
    """the bytes of state one unit moves through HBM in one pass: the gathers and write-backs of every segment, from the host tables' segment table (the
    record's bytes are sample_tiled_info's bytes_per_job)"""
    from class_sweep_rate import CODES
    lib = C.CDLL(os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc", "build", "libqecmc_tables.so"))
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    lib.qt_class_sweep_tiled_info.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.c_char_p, C.c_int]
    lib.qt_class_sweep_tiled_segments.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u32p, C.c_int]
    v = np.zeros(16, np.int32)
    assert lib.qt_class_sweep_tiled_info(CODES[name], L, 0, 0, v.ctypes.data_as(i32p), None, 0) == 0
    seg = np.zeros(8 * int(v[8]), np.uint32)
    assert lib.qt_class_sweep_tiled_segments(CODES[name], L, 0, 0, seg.ctypes.data_as(u32p), seg.size) == seg.size
    state = 0
    for op_first, op_count, tile, live, live_in, live_out, n_tiles, _ in seg.reshape(-1, 8).tolist():
        state += 8 * n_tiles * ((1 << bin(live_in & tile).count("1")) * (live_in != 0 or op_first != 0) + (1 << bin(live_out & tile).count("1")) * (live_out != 0))
    return state


def calls_of(lib, name, L, n, K=1, mode=0, record_bytes=0):
    """(sample, sweep, buffers): the two calls of one case on the same chains, of the library `lib` -- sample is None where the library has no sampler --, and
    the arrays the calls read and write, (chains, weights, z, chain_out, class_out): the caller holds them for as long as it makes the calls"""
    from class_sweep_rate import CODES, random_chains
    from qecmc import _lib as L_
    from qecmc.exact import depolarizing_w4
    code = CODES[name]
    flat = random_chains(name, L, n).reshape(n, -1)
    ncls = 16 if name == "toric" else 4
    w = np.ascontiguousarray(depolarizing_w4(P))
    f64p = C.POINTER(C.c_double)
    z = np.zeros((n, ncls))
    out, cls = np.zeros((n, K, flat.shape[1]) if mode else (n, ncls, K, flat.shape[1]), np.uint8), np.zeros((n, K), np.int32)
    buffers = (flat, w, z, out, cls)

    def sweep():
        L_.check(lib.qecmc_class_sweep_tiled(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), 0, 0, z.ctypes.data_as(f64p), None))

    def sample():
        L_.check(lib.qecmc_class_sample_tiled(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), 0, 0, record_bytes, K, 1234, 0, mode, L_.u8(out), L_.i32(cls),
                                              z.ctypes.data_as(f64p)))
    return (sample if hasattr(lib, "qecmc_class_sample_tiled") else None), sweep, buffers


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
    """the library at `path` with the argtypes of qecmc_class_sweep_tiled alone (a build that lacks the sampler's entry points)"""
    from qecmc import _lib as L_
    lib = C.CDLL(os.path.abspath(path))
    lib.qecmc_class_sweep_tiled.restype = C.c_int
    lib.qecmc_class_sweep_tiled.argtypes = L_.lib().qecmc_class_sweep_tiled.argtypes
    lib.qecmc_last_error.restype = C.c_char_p
    return lib


def measure(repeats, other):
    import torch
    import qecmc
    from qecmc import _lib as L_
    from qecmc.exact import sample_tiled_info, sweep_tiled_info
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the times are measured on the device or not at all")
    torch.cuda.init()
    prop = torch.cuda.get_device_properties(0)
    rows = []
    for name, L, n in CASES:
        inf, sinf = sweep_tiled_info(name, L), sample_tiled_info(name, L)
        state = segment_bytes(name, L)
        sample, sweep, buffers = calls_of(L_.lib(), name, L, n)
        a, b = alternate(torch, sample, sweep, repeats)
        row = dict(code=name, L=L, N=n, width=inf["width"], held=inf["held"], segments=inf["segments"], ncls=inf["ncls"], n_forget=sinf["n_forget"],
                   bytes_per_job=sinf["bytes_per_job"], jobs_per_pass=sinf["jobs_per_pass"], state_bytes_per_unit=state,
                   byte_ratio=(state + sinf["bytes_per_job"]) / state, expected_call_ratio=1.0 + (state + sinf["bytes_per_job"]) / state)
        row.update(stats("sample_call", a)); row.update(stats("sweep_call", b))
        row.update(sample_over_sweep_call=row["sample_call_ms_median"] / row["sweep_call_ms_median"], larger_spread_ms=max(max(a) - min(a), max(b) - min(b)))
        for K in KS:
            at_k, _, buffers_k = calls_of(L_.lib(), name, L, n, K=K)
            c, d = alternate(torch, at_k, sample, repeats)
            row.update(stats("sample_call_K%d" % K, c))
            row["walk_us_per_sample_K%d" % K] = 1e3 * (float(np.median(c)) - float(np.median(d))) / ((K - 1) * n * inf["ncls"])
        if other:
            _, theirs, their_buffers = calls_of(other_library(other), name, L, n)
            c, d = alternate(torch, sweep, theirs, repeats)
            row.update(stats("this_build_sweep_call", c)); row.update(stats("other_build_sweep_call", d))
            row.update(this_over_other=float(np.median(c)) / float(np.median(d)), other_larger_spread_ms=max(max(c) - min(c), max(d) - min(d)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows, dict(name=prop.name, compute_units=int(prop.multi_processor_count))


def past_the_cap(skip):
    """one posterior call at rotated L = 21 under record_bytes = 40 GiB, where the card has the memory free"""
    import torch
    from qecmc import _lib as L_
    from qecmc.exact import sample_tiled_info
    free, total = torch.cuda.mem_get_info()
    inf = sample_tiled_info("rotated", 21, record_bytes=40 << 30)
    row = dict(code="rotated", L=21, N=1, K=1, mode=1, record_bytes=40 << 30, bytes_per_job=inf["bytes_per_job"], free_bytes_before=int(free))
    if skip or free < (48 << 30):
        row["ran"] = False
        row["why"] = "skipped on the command line" if skip else "less than 48 GiB free on the card"
        return row
    sample, _, (_, _, z, out, cls) = calls_of(L_.lib(), "rotated", 21, 1, K=1, mode=1, record_bytes=40 << 30)
    t0 = time.time()
    row["call_ms"] = event_ms(torch, sample)
    row.update(ran=True, wall_s=time.time() - t0, cls=int(cls[0, 0]), errors=int(np.count_nonzero(out[0, 0])), z=[float(x) for x in z[0]],
               free_bytes_after=int(torch.cuda.mem_get_info()[0]))
    print(json.dumps(row), flush=True)
    return row


def purpose():
    import qecmc
    name, L, n, steps, burn = PURPOSE
    rng = np.random.default_rng(85)
    err = np.zeros((n, L, L), np.uint8)
    hit = rng.random(err.shape) < P
    err[hit] = rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)
    exact = qecmc.posterior_error_counts(name, err, P, 1024, seed=20261021, method="tiled")
    rows = []
    for scan in ("random", "wave"):
        kw = dict(Nc=5, iters=10, tops_burn=0, code=qecmc.ROTATED, scan=scan, return_swap_stats=True, seed=77)
        a = qecmc.pteq_batch(err, P, steps=burn, **kw)
        b = qecmc.pteq_batch(err, P, steps=burn + steps, **kw)
        mcmc = (b["nerr_sums"][:, 0].astype(np.int64) - a["nerr_sums"][:, 0]) / steps
        d = mcmc - exact
        bar = d.std(ddof=1) / np.sqrt(len(d))
        rows.append(dict(code=name, L=L, N=n, p=P, scan=scan, steps=steps, burn=burn, exact_mean=float(exact.mean()), sampler_mean=float(mcmc.mean()), mean_d=float(d.mean()),
                         bar=float(bar), mean_d_in_bars=float(abs(d.mean()) / bar)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_sample_tiled_rate.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--skip-l21", action="store_true")
    a = ap.parse_args()
    if a.repeats < 5:
        sys.exit("--repeats: a median of at least 5")
    rows, dev = measure(a.repeats, a.other_lib)
    res = dict(device=dev, cases=rows, purpose=purpose(), past_the_cap=past_the_cap(a.skip_l21), note=NOTE)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
