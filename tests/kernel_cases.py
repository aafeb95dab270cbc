"""One parity case per built kernel: the registry behind tests/test_kernel_cases_cpu.py and the by-hand GPU run below.

tests/kernel_cases.json is the table -- committed data, one row per ladder / wave / colour / statistics / shortest-chain kernel of libqecmc, keyed by the
label tools/kernel_resources.py gives the kernel.  A row names the Python call that makes the library run that kernel: the entry point (`entry`), the
code, L, Nc, the batch N, steps, iters, the noise (p -- pz_tilde under the alpha rule --, eta, alpha), p_logical, the scan, whether the criterion runs
(`conv`; SEQ = 1, TOPS = 3, eps = 0.6 as tests/fuzz_gpu.py), whether final states are asked for (`states`), first_syndrome, the developer switches
and the persistent grid of qecmc_params.flags, the seed.  tools/derive_kernel_cases.py proposes the table from the CPU sweep when kernels are added;
nothing regenerates it at test time.

What this module does with a row:
  predict(T, case)    the kernel the library will launch, on the host: plan_host() on the case's real parameter block (qt_plan) plus the launch mode
                      its entry point presents (work queue, statistics, unique-chain set, Chain_xyz), fed to choose_kernel() (qt_choose_kernels)
  run_gpu(q, case)    the call itself
  run_oracle(case)    the CPU oracle on the same Philox streams
  differences(...)    the fields that differ -- bit for bit, no tolerance
  vacuous(...)        why the oracle's run would prove nothing (conditions on the reference alone)

`python tests/kernel_cases.py --oracle [label-substring]` runs the oracle half and the non-vacuity conditions of the cases without a GPU, with the
seconds each takes; `--gpu [label-substring]` runs them as tests/test_gpu_kernel_cases.py does and stops at the first HIP error.  On the larger lattices
the rows use a noisy bottom rung (p = 0.3 .. 0.6) and runs of 1 000 .. 6 000 steps: at p = 0.1 no ladder's flag comes back to the top there."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:          # (run as a script or from tools/: hostlib is a sibling)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hostlib import ROOT, SEALED_HEADS, kernel_resources, resource_rows, tables_lib          # noqa: E402
from hostlib import KERNEL_SHAPE_FIELDS as FIELDS          # noqa: E402
from qecmc import _lib as L_            # noqa: E402

TABLE = os.path.join(ROOT, "tests", "kernel_cases.json")
CODES = ["toric", "xzzx", "rotated", "planar"]
SCANS = ["random", "sweep", "colour", "wave"]
ENTRIES = ("pteq", "pteq_stats", "ptdc", "shortest")
CRITERION = dict(SEQ=1, TOPS=3, eps=0.6)          # loose, as tests/fuzz_gpu.py: ladders stop within the horizon
TOPS_BURN = 1
SET_CAPACITY = 1024                               # pteq_shortest_batch's default: distinct keys a ladder's set holds
XYZ = (0.04, 0.03, 0.05)                          # Chain_xyz sampling rates (ptdc, xyz = 1)
# the ladders whose statistics the Python-stepped oracles compute (both ends of the first wavefront, the second one's first and last live lane)
STAT_LADDERS = (0, 1, 33, 63, 64, 69)


def load_cases():
    with open(TABLE) as f:
        cases = json.load(f)
    labels = [c["label"] for c in cases]
    assert len(set(labels)) == len(labels), "a kernel has two cases"
    return cases


def built_labels():
    """the labels of every ladder / wave / colour / statistics / shortest-chain kernel in csrc/build/*.res"""
    return sorted({r["label"] for r in resource_rows() if r["label"].startswith(SEALED_HEADS)})


# ------------------------------------------------------------------------------------------------------------------ the parameter block and the prediction
def noise_of(case):
    return L_.NOISE_ALPHA if case["alpha"] else L_.NOISE_BIASED if case["eta"] else L_.NOISE_DEPOLARIZING


def params_of(case):
    """the parameter block the case's entry point hands the library (qecmc/decoders.py pteq_batch / ptdc_batch, decoders_biasednoise.py pteq_shortest_batch)"""
    code, scan = CODES.index(case["code"]), SCANS.index(case["scan"])
    if case["entry"] == "ptdc":         # ptdc_batch: the sampling ladder without logical moves, fixed length (qecmc_ptdc_batch_xyz)
        return L_.make_params(code=code, L=case["L"], Nc=case["Nc"], p=sum(XYZ) if case["xyz"] else case["p"], iters=case["iters"], steps=case["steps"],
                              seed=case["seed"], first_syndrome=case["first_syndrome"], noise=noise_of(case), alpha=case["alpha"] or 0.0)
    return L_.make_params(code=code, L=case["L"], Nc=case["Nc"], p=case["p"], p_logical=case["p_logical"], iters=case["iters"], steps=case["steps"],
                          tops_burn=TOPS_BURN, seed=case["seed"], first_syndrome=case["first_syndrome"], scan=scan, noise=noise_of(case),
                          eta=case["eta"] or 0.0, alpha=case["alpha"] or 0.0, conv_mode=L_.CONV_ERROR_BASED if case["conv"] else L_.CONV_NONE,
                          flags=L_.dev_flags(case["switches"], case["queue_grid"]), **CRITERION)


def predict(T, case, cu_count=256):
    """the label of the kernel the case's launch runs, "refused: why" where the chooser builds none for it, "no plan: why" where plan_host() makes no plan,
    "no launch: why" where the entry point refuses before it launches"""
    shape, msg, lds, grid = np.zeros(len(FIELDS), dtype=np.int32), C.create_string_buffer(600), C.c_uint64(), C.c_uint32()
    pr = params_of(case)
    if T.qt_plan(C.byref(pr), cu_count, shape.ctypes.data, C.byref(lds), C.byref(grid), msg, len(msg)):
        return "no plan: " + msg.value.decode()
    s = dict(zip(FIELDS, (int(x) for x in shape)))
    entry = case["entry"]
    # a criterion launch runs on the plan's persistent grid unless it asks for final states or statistics (qecmc_pteq_launch_dev)
    wants = bool(case["states"]) or entry in ("pteq_stats", "shortest")
    takes = bool(T.qt_launch_takes_queue(grid.value, case["steps"], int(wants)))
    if entry == "ptdc":
        s.update(uset=1, xyz=int(case["xyz"]))
    elif entry == "pteq_stats":
        s.update(stats=1)
    elif entry == "shortest":
        s.update(stats=2)
    elif case["scan"] == "wave":
        if case["conv"] and not takes:
            return "no launch: scan = wave runs the criterion on its persistent grid only"
    else:
        s.update(queue=int(takes))          # (scan = wave: its own queue, no counter offered)
    key = np.zeros(11, dtype=np.int64)
    T.qt_choose_kernels(np.array([s[f] for f in FIELDS], dtype=np.int32).ctypes.data, 1, key.ctypes.data)
    if key[0] == 0:
        return "refused: " + C.string_at(int(key[10])).decode()
    return kernel_resources.key_label(key)


# ------------------------------------------------------------------------------------------------------------------ inputs
def state_shape(case):
    L = case["L"]
    return (2, L, L) if case["code"] in ("toric", "planar") else (L, L)


def make_init(case):
    """the seeds of the batch, drawn from the case's seed: errors at rate p_init (ptdc: one representative per class and syndrome)"""
    rng = np.random.default_rng(case["seed"])
    shape = (case["N"],) + state_shape(case)
    m = np.zeros(shape, np.uint8)
    err = rng.random(shape) < case["p_init"]
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    if case["code"] == "planar":
        m[:, 1, -1, :] = 0; m[:, 1, :, -1] = 0                       # (the idle row and column of layer 1)
    m.setflags(write=False)
    if case["entry"] != "ptdc":
        return m
    from oracle import oracle as orc
    if case["code"] == "toric":
        reps = np.stack([np.stack([orc.toric_to_class(x, e) for e in range(16)]) for x in m])
    else:
        ocode = getattr(orc, case["code"].upper())
        reps = np.stack([np.stack([orc.surf_apply_logical(ocode, x, op)[0] for op in range(4)]) for x in m])
    reps.setflags(write=False)
    return reps


# ------------------------------------------------------------------------------------------------------------------ the two halves
def _rule(case, for_oracle):
    if case["alpha"]:
        return dict(noise=2, alpha=case["alpha"], det_pow=1) if for_oracle else dict(alpha=case["alpha"])
    if case["eta"]:
        return dict(noise=1, eta=case["eta"]) if for_oracle else dict(eta=case["eta"])
    return {}


def run_gpu(q, case, init):
    code = getattr(q, case["code"].upper())
    flags = q.dev_flags(case["switches"], case["queue_grid"])
    crit = dict(conv_criteria="error_based" if case["conv"] else None, **CRITERION)
    common = dict(Nc=case["Nc"], steps=case["steps"], iters=case["iters"], seed=case["seed"], first_syndrome=case["first_syndrome"], code=code)
    if case["entry"] == "ptdc":
        p = np.array(XYZ) if case["xyz"] else case["p"]
        n, m = q.ptdc_batch(init, p, with_m=True, alpha=case["alpha"], **common)
        return dict(hist=n, mhist=m)
    if case["entry"] == "shortest":
        return q.pteq_shortest_batch(init, case["p"], case["alpha"], tops_burn=TOPS_BURN, p_logical=case["p_logical"], scan=case["scan"], flags=flags,
                                     **crit, **common)
    return q.pteq_batch(init, case["p"], tops_burn=TOPS_BURN, p_logical=case["p_logical"], scan=case["scan"], flags=flags,
                        return_states=bool(case["states"]), return_swap_stats=case["entry"] == "pteq_stats", **crit, **_rule(case, False), **common)


def run_oracle(case, init):
    from oracle import oracle as orc
    ocode, scan = getattr(orc, case["code"].upper()), SCANS.index(case["scan"])
    common = dict(iters=case["iters"], seed=case["seed"], first_syndrome=case["first_syndrome"])
    if case["entry"] == "ptdc":
        p = np.array(XYZ) if case["xyz"] else case["p"]
        n, m = orc.ptdc_batch(ocode, init, p, case["Nc"], case["steps"], with_m=True, alpha=case["alpha"], **common)
        return dict(hist=n, mhist=m)
    crit = dict(conv_criteria="error_based", **CRITERION) if case["conv"] else {}
    if case["entry"] == "shortest":
        import util_shortest_batch as U
        rows = [U._one(ocode, init[l], case["p"], case["alpha"], case["Nc"], case["steps"], case["iters"], scan, bool(case["conv"]), CRITERION["SEQ"],
                       CRITERION["TOPS"], TOPS_BURN, CRITERION["eps"], case["seed"], case["first_syndrome"] + l) for l in range(case["N"])]
        out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
        return out
    if case["scan"] == "wave" and case["conv"]:
        # the criterion runs of scan = wave take the deterministic per-workgroup queue: the oracle's restatement of it, on the grid the launch uses
        groups = (case["N"] + 63) // 64
        grid = max(1, min(case["queue_grid"] or groups, groups))
        kw = {k: v for k, v in _rule(case, True).items() if k != "eta"}
        assert kw.pop("noise", 0) in (0, 2)
        return orc.pteq_wave_queue(ocode, init, case["p"], case["Nc"], case["steps"], grid, tops_burn=TOPS_BURN, noise=2 if case["alpha"] else 0, **kw,
                                   **CRITERION, **common)
    ref = orc.pteq_batch(ocode, init, case["p"], case["Nc"], case["steps"], tops_burn=TOPS_BURN, return_states=not case["conv"], scan=scan, **crit,
                         **_rule(case, True), **common)
    if case["entry"] == "pteq_stats":
        # the oracle's ladder keeps both counters: stepped from Python, on the ladders of STAT_LADDERS
        rule = _rule(case, True)
        acc, nsum = {}, {}
        for s in (l for l in STAT_LADDERS if l < case["N"]):
            ld = orc.Ladder(ocode, init[s], case["p"], case["Nc"], case["p_logical"], scan=scan, **rule)
            rng = orc.Rng.philox(case["seed"], case["first_syndrome"] + s)
            for _ in range(int(ref["steps_done"][s])):          # (a criterion run counts up to the step it stops at)
                ld.step(case["iters"], rng)
            acc[s], nsum[s] = ld.swap_accepts.astype(np.uint32), ld.nerr_sums.astype(np.uint32)
        ref["swap_accepts"], ref["nerr_sums"] = acc, nsum
    if case["scan"] == "colour" and not case["conv"]:
        # a fixed-length run of scan = colour reports the first step with tops0 >= TOPS in steps_done / converged (tests/test_gpu_colour.py): the oracle's
        # ladders stepped from Python say which
        reached = np.zeros(case["N"], dtype=np.uint64)
        for l in range(case["N"]):
            ld = orc.Ladder(ocode, init[l], case["p"], case["Nc"], case["p_logical"], scan=scan, **_rule(case, True))
            rng = orc.Rng.philox(case["seed"], case["first_syndrome"] + l)
            for t in range(case["steps"]):
                ld.step(case["iters"], rng)
                if ld.tops0 >= CRITERION["TOPS"]:
                    reached[l] = t + 1
                    break
        ref["steps_done"], ref["converged"] = np.where(reached > 0, reached, case["steps"]), reached > 0
    return ref


def differences(case, got, ref):
    """the compared fields in which the library's answer differs from the oracle's (bit for bit)"""
    bad = []
    if case["entry"] == "ptdc":
        return [k for k in ("hist", "mhist") if not np.array_equal(got[k], ref[k])]
    for k in ("counts", "samples", "tops0", "steps_done", "converged"):
        if not np.array_equal(np.asarray(got[k]).astype(np.uint64), np.asarray(ref[k]).astype(np.uint64)):
            bad.append(k)
    if case["entry"] == "shortest":
        for k in ("shortest", "shortest_n", "unique_n"):
            if not np.array_equal(np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)):
                bad.append(k)
        if not np.array_equal(np.asarray(got["overflow"]).astype(bool), np.asarray(ref["offered"]) > SET_CAPACITY):
            bad.append("overflow")
        return bad
    if not case["conv"] and case["states"] and not np.array_equal(got["states"], ref["states"]):
        bad.append("states")
    if case["entry"] == "pteq_stats":
        for k in ("swap_accepts", "nerr_sums"):
            if any(not np.array_equal(got[k][s], v) for s, v in ref[k].items()):
                bad.append(k)
    return bad


def vacuous(case, init, ref):
    """why the oracle's run of the case would prove nothing -- [] when it proves something.  Conditions on the reference alone."""
    why = []
    if case["entry"] == "ptdc":
        # unique-chain sets: at least two distinct configurations counted in some class
        if not (ref["hist"].reshape(-1, ref["hist"].shape[-1]).sum(axis=1) >= 2).any():
            why.append("no set holds two distinct configurations")
        return why
    if case["entry"] == "shortest":
        if not (ref["unique_n"].max(axis=1) >= 2).any():
            why.append("no class of any ladder counted two distinct configurations")
        if (ref["offered"] > SET_CAPACITY).any():          # (an overflowed ladder's unique_n row is unspecified)
            why.append("a ladder overflows the default set")
    if not np.asarray(ref["samples"]).sum() > 0:
        why.append("samples == 0 everywhere")
    if not (np.asarray(ref["tops0"]) > 0).any():
        why.append("tops0 == 0 in every ladder")
    if case["conv"]:
        conv = np.asarray(ref["converged"]).astype(bool)
        if not (conv & (np.asarray(ref["steps_done"]) < case["steps"])).any():
            why.append("no ladder converges before the horizon")
        if "queue" in case["label"] and case["N"] < 3 * 64 * max(case["queue_grid"], 1):
            why.append("fewer than three refill rounds of a lane")
    elif "states" in ref:
        moved = (ref["states"][:, 0].reshape(case["N"], -1) != np.asarray(init).reshape(case["N"], -1)).any(axis=1)
        if 2 * int(moved.sum()) < case["N"]:
            why.append("the bottom rung ends where it started in more than half of the ladders")
    return why


_cached_tables = tables_lib          # (hostlib keeps one handle per path)


def main_gpu(argv):
    import qecmc as q
    bad = 0
    for c in (c for c in load_cases() if len(argv) < 2 or argv[1] in c["label"]):
        init = make_init(c)
        try:
            got = run_gpu(q, c, np.array(init))
        except q.QecmcError as e:
            print("ERROR %s %s" % (c["label"], e), flush=True)
            bad += 1
            if "libqecmc error -3" in str(e):
                print("a HIP call failed: nothing more is started on the GPU")
                break
            continue
        ran = q._lib.last_kernel()
        ref = run_oracle(c, init)
        diff, why = differences(c, got, ref), vacuous(c, init, ref)
        ok = ran == c["label"] and not diff and not why
        bad += not ok
        print("%-8s %-64s %s" % ("ok" if ok else "MISMATCH", c["label"], "" if ok and not why else dict(ran=ran, differs=diff, vacuous=why)), flush=True)
    print("%d bad" % bad)
    return 1 if bad else 0


def main(argv):
    if argv and argv[0] == "--gpu":
        return main_gpu(argv)
    if not argv or argv[0] != "--oracle":
        sys.exit(__doc__)
    cases = [c for c in load_cases() if len(argv) < 2 or argv[1] in c["label"]]
    T, bad, t0 = _cached_tables(), 0, time.time()
    for c in cases:
        t = time.time()
        pred = predict(T, c)
        init = make_init(c)
        why = vacuous(c, init, run_oracle(c, init))
        ok = pred == c["label"] and not why
        bad += not ok
        print("%-4s %5.2f s  %-64s %s" % ("ok" if ok else "BAD", time.time() - t, c["label"], "" if ok else (pred, why)), flush=True)
    print("%d cases, %d bad, %.0f s" % (len(cases), bad, time.time() - t0))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
