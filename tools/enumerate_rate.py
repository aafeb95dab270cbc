#!/usr/bin/env python3
"""Rates of the coset enumeration (qecmc_coset_enumerate) -> profiles/enumerate_rate.json.

    GPU box:  python3 tools/enumerate_rate.py [--out profiles/enumerate_rate.json] [--repeats 7] [--kernel-stats kernel_stats.csv]
              rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/enumerate_rate.py --trace-only
              (a run of its own; its *_kernel_stats.csv goes to --kernel-stats of a plain run)

Per case -- xzzx L = 5 with N = 1 and N = 64, toric L = 3 with N = 4096, planar L = 4 with N = 16 (one launch that fills the pair budget) -- the time of
one warm call between two device events on the null stream (H2D of the chains' representatives, the zeroing, every launch, D2H of the histograms),
median and spread of `repeats`, and class-elements per second from the median; the same call on ONE chunk of 2^8 elements (the copies and the launch
overhead alone); the kernel's own times from a kernel trace where one is given; the C++ twin's and the NumPy enumerator's rates on this host's CPU;
and the inner loop's instruction count from `hipcc -S` with the VALU-issue bound it implies.  No GPU: the script fails."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"))
CSRC = os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc")
CASES = [("xzzx", 5, 1), ("xzzx", 5, 64), ("toric", 3, 4096), ("planar", 4, 16)]


def random_chains(code, L, n, seed=0):
    rng = np.random.default_rng([17, L, n, seed])
    shape = (n, 2, L, L) if code in ("toric", "planar") else (n, L, L)
    m = np.zeros(shape, dtype=np.uint8)
    err = rng.random(shape) < 0.15
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    if code == "planar":
        m[:, 1, -1, :] = 0
        m[:, 1, :, -1] = 0
    return m


def timed_call(lib, L_, torch, code, L, flat, hist, chunk_bits, first, count, repeats):
    """ms between two device events around one call, after a warm-up: [repeats]"""
    def call():
        L_.check(lib.qecmc_coset_enumerate(code, L, len(flat), L_.u8(flat), chunk_bits, first, count, hist.ctypes.data_as(L_._u64p), None))
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


def gpu_cases(repeats, trace_only, library=None):
    import torch
    import qecmc
    from qecmc import _lib as L_
    from qecmc.exact import enumerator_info
    if library:
        L_.use_library(library)
    if qecmc.device_count() < 1:
        sys.exit("no GPU visible: the rates are measured on the device or not at all")
    lib = L_.lib()
    torch.cuda.init()
    prop = torch.cuda.get_device_properties(0)
    rows = []
    for name, L, n in CASES:
        code, inf = {"toric": 0, "xzzx": 1, "rotated": 2, "planar": 3}[name], enumerator_info(name, L)
        flat = random_chains(name, L, n).reshape(n, -1)
        hist = np.zeros((n, inf["ncls"], inf["nq"] + 1, inf["nq"] + 1), dtype=np.uint64)
        if trace_only:
            L_.check(lib.qecmc_coset_enumerate(code, L, n, L_.u8(flat), 0, 0, 0, hist.ctypes.data_as(L_._u64p), None))
            continue
        full = timed_call(lib, L_, torch, code, L, flat, hist, 0, 0, 0, repeats)
        assert np.all(hist.sum(axis=(2, 3)) == 1 << inf["rank"])
        small = timed_call(lib, L_, torch, code, L, flat, hist, 8, 0, 1, repeats)
        work = n * inf["ncls"] * (1 << inf["rank"])
        med = float(np.median(full))
        rows.append(dict(code=name, L=L, N=n, rank=inf["rank"], ncls=inf["ncls"], chunk_bits=inf["chunk_bits"], class_elements=work,
                         launches=-(-n // min(n, 1024, max(1, (1 << 28) >> inf["chunk_bits"]))) << (inf["rank"] - inf["chunk_bits"]),
                         call_ms_median=med, call_ms_min=float(min(full)), call_ms_max=float(max(full)),
                         class_elements_per_s_of_the_call=work / (med * 1e-3),
                         one_chunk_of_256_call_ms_median=float(np.median(small)), hist_bytes=int(hist.nbytes)))
    return rows, dict(name=prop.name, compute_units=int(prop.multi_processor_count))


def cpu_rates():
    """class-elements per second of the C++ twin (the host-table test library, g++ -O1, one thread) and of the NumPy meet-in-the-middle enumerator of the
    tests, on one xzzx L = 5 syndrome"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    subprocess.check_call(["make", "-C", CSRC, "-s", "tables"])
    T = C.CDLL(os.path.join(CSRC, "build", "libqecmc_tables.so"))
    flat = random_chains("xzzx", 5, 1).reshape(1, -1)
    hist = np.zeros((1, 4, 26, 26), dtype=np.uint64)
    T.qt_coset_enumerate.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    t0 = time.perf_counter()
    assert T.qt_coset_enumerate(1, 5, 1, flat.ctypes.data, 0, 0, 0, hist.ctypes.data, None) == 0
    twin_s = time.perf_counter() - t0
    out = dict(twin_seconds_per_syndrome=twin_s, twin_class_elements_per_s=4 * (1 << 24) / twin_s)
    try:
        import types
        from oracle import oracle as orc
        from util_exact import PlaquetteWeightEnumerator
        api = types.SimpleNamespace(apply_stabilizer=orc.surf_apply_stabilizer, apply_logical=orc.surf_apply_logical, eq_class=orc.surf_eq_class,
                                    ngen=orc.surf_ngen, gen_rco=orc.surf_gen_rco)
        t0 = time.perf_counter()
        e = PlaquetteWeightEnumerator(orc.XZZX, flat.reshape(5, 5), api)
        numpy_s = time.perf_counter() - t0
        assert np.array_equal(e.H.astype(np.uint64), hist[0])
        out.update(numpy_seconds_per_syndrome=numpy_s, numpy_class_elements_per_s=4 * (1 << 24) / numpy_s)
    except ImportError as err:                                                # (the CPU oracle of the source tree is not built here)
        out.update(numpy_seconds_per_syndrome=None, note="NumPy enumerator not measured: %s" % err)
    return out


def inner_loop(dev):
    """VALU and LDS instructions per class-element of k_enumerate<4, 6>, between the first and the last LDS add of its unrolled walk (`hipcc -S`), and
    the bound the VALU issue rate implies: 4 SIMDs x 16 lanes per clock and CU at the peak engine clock"""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "enumerate.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", asm,
                               os.path.join(CSRC, "enumerate.hip")], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    body = text[text.index("_ZN5qecmc11k_enumerateILi4ELi6E"):]
    body = body[body.index(":\n"):body.index(".Lfunc_end")]
    lines = [ln.strip() for ln in body.splitlines() if re.match(r"\s+[a-z]", ln)]
    adds = [i for i, ln in enumerate(lines) if ln.startswith("ds_add_u32")]
    region = lines[adds[0] + 1:adds[-1] + 1]
    n = len(adds) - 1
    valu, salu, lds = (sum(ln.startswith(p) for ln in region) / n for p in ("v_", "s_", "ds_"))
    out = dict(lds_adds_in_the_walk=len(adds), valu_per_class_element=valu, salu_per_class_element=salu, lds_per_class_element=lds)
    out["valu_issue_bound_class_elements_per_s"] = dev["compute_units"] * 64 * dev["peak_clock_mhz"] * 1e6 / valu
    return out


def kernel_stats(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_enumerate" in r["Name"]]
    return [dict(kernel=r["Name"], calls=int(r["Calls"]), average_ms=float(r["AverageNs"]) / 1e6, max_ms=float(r["MaxNs"]) / 1e6,
                 total_ms=float(r["TotalDurationNs"]) / 1e6) for r in rows]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enumerate_rate.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernel-stats", default=None, help="*_kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --trace-only")
    ap.add_argument("--peak-clock-mhz", type=float, default=2400.0, help="the peak engine clock the VALU-issue bound is stated at (MI355X: 2400)")
    ap.add_argument("--library", default=None, help="another build of libqecmc.so to measure (an A/B of two builds: one process each, alternating)")
    ap.add_argument("--trace-only", action="store_true", help="run every case once, untimed (the workload of a kernel trace)")
    a = ap.parse_args()
    rows, dev = gpu_cases(a.repeats, a.trace_only, a.library)
    if a.trace_only:
        sys.exit(0)
    dev["peak_clock_mhz"] = a.peak_clock_mhz
    res = dict(library=a.library or "in-tree", device=dev, cases=rows, cpu=cpu_rates(), inner_loop=inner_loop(dev),
               kernel_trace=kernel_stats(a.kernel_stats) if a.kernel_stats else "not measured",
               note="call_ms: device events around one qecmc_coset_enumerate call (copies included); the trace-only workload runs each case once, so a "
                    "kernel's total_ms over the trace is the kernel time of the four cases together")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
