"""The samplers at the ends of their parameter range: the one table behind tests/test_sampler_range_cpu.py (the plans' flags, the tables' saturation and the
conditions on the oracle alone, no GPU) and tests/test_gpu_sampler_range.py (the kernels, bit for bit against the oracle on the same Philox streams).

The sampler kernels branch at run time on what the plan says of the noise parameters (csrc/plan_host.hpp):

  A  swap_fast_ok = 0: a swap threshold at d = 1 no longer fits 32 bits -- p = 0.75 with two or more rungs (the rungs coincide, p_diff = 1, and every rung
     takes the coin: lower_acc = 1), and p so close below 0.75 that p_diff > 1 - 2^-32 (lower_acc = 0).  The ladder kernels then compare 64-bit words
     against the plan's table in global memory, the colour kernels carry two-word thresholds in another LDS carve, scan = wave is refused.
  B  bias_f32ok, a bit per rung under the biased and alpha rules: on iff iters <= 512 and 4 iters max|log2 ratio| <= 2000.  Off, the fast acceptance
     estimate takes the double-precision route; the wave kernels of the alpha rule are refused.
  C  low p under the depolarizing rule: ceil(f^d 2^32) and ceil(f^d 2^44) saturate at 1 (at 0 once f^d underflows), the top rung's row and the swap rows go
     flat, swap_inv_log2 shrinks to 0.  Where f^4 underflows (p below about 3.7e-81) scan = sweep and scan = colour are refused by name.

A row names the call (entry), the code, L, Nc, the batch N, steps, iters, the scan, the noise (p -- pz_tilde under the alpha rule --, eta, alpha), the seed
and the PREMISE it is there for: the plan's flags (`flags`: swap_fast_ok, top_acc, lower_acc), the per-rung mask (`f32`: "on", "off", "mixed" = hot rungs
on and cold rungs off), a named refusal (`refusal`), or -- group C -- the saturation (`sat`).  Nothing here says what the flags ARE: the CPU file reads
them from plan_host() and holds them against the premise.  p may be symbolic: "thr32" / "thr44" are the largest p with ceil(f^4 2^32) == 1 /
ceil(f^4 2^44) == 1, found by bisection on the plan's own tables (edge_p()); "min" is the smallest positive double.  `weaker` names a condition of
vacuous() the row cannot meet, with the reason, and what is asserted in its place.  Seeds, steps and the start density P_INIT were chosen so that the
oracle alone meets the conditions (the CPU file checks it); chains start from a dense error, independent of the sampling p, so the cold rungs have
somewhere to go."""
import ctypes as C
import functools

import numpy as np

from hostlib import tables_lib            # (puts the repository and the package on sys.path)
from qecmc import _lib as L_

CODES = ["toric", "xzzx", "rotated", "planar"]
SCANS = ["random", "sweep", "colour", "wave"]
P_INIT = 0.4                               # (at 0.15 and 0.3 the start is a local minimum of most L = 3 and 5 ladders: their cold rungs never left it)
NO_SSW = 8                                 # qecmc_params.flags bit: the replay form of the wave kernels' cascade (tests/test_gpu_wave_bounds.py)
MIN_DOUBLE = 5e-324
CONV_TOPS_BURN = 1                         # tops_burn of the criterion row
TOPS = 10                                  # pteq_batch's default: a fixed-length run of scan = colour reports the first step with tops0 >= TOPS
ALL_ACCEPTED_075 = "p = 0.75: the rungs coincide, p_diff = 1 and u < 1 always -- every swap is accepted"
ALL_ACCEPTED_NEAR = "p_diff^d > 1 - 2^-24 for every d <= nq: a refusal needs a uniform within 2^-24 of 1, and the run draws none"
ALL_ACCEPTED_NEIGHBOUR = "p_diff^d > 1 - 2^-21 for every d <= nq: a refusal needs a uniform within 2^-21 of 1, and the run draws none"
NEAR_BITS = {ALL_ACCEPTED_NEAR: 24, ALL_ACCEPTED_NEIGHBOUR: 21}          # (held against the plan's swap rows in tests/test_sampler_range_cpu.py)
ALPHA_TOP = "the alpha rule's top rung sits at pz_tilde = 1: every weight ratio is 1 and every proposal is accepted"


def _r(id, group, entry, code, L, Nc, N, steps, iters, scan, seed, p, eta=None, alpha=None, **premise):
    assert code in CODES and scan in SCANS and entry in ("pteq", "pteq_stats", "pteq_conv", "step", "chain", "ptdc")
    row = dict(id=id, group=group, entry=entry, code=code, L=L, Nc=Nc, N=N, steps=steps, iters=iters, scan=scan, seed=seed, p=p, eta=eta, alpha=alpha,
               first_syndrome=64 if scan == "wave" else 3, weaker={}, forms=(0, NO_SSW) if scan == "wave" else (0,))
    row.update(premise)
    return row


ON = dict(swap_fast_ok=1, top_acc=1, lower_acc=0)             # an ordinary depolarizing ladder
COIN = dict(swap_fast_ok=0, top_acc=1, lower_acc=1)           # p = 0.75: every rung takes the coin
NEAR = dict(swap_fast_ok=0, top_acc=1, lower_acc=0)           # just below: the thresholds of d = 1 leave 32 bits, the lower rungs still test
TABLE = dict(swap_fast_ok=1, top_acc=0, lower_acc=0)          # the table-driven rules
COLOUR_ALPHA = dict(swap_fast_ok=1, top_acc=1, lower_acc=0)   # ... scan = colour: the alpha rule's top rung takes the coin
P_NEAR, P_NEIGHBOUR = 0.75 - 1e-11, 0.75 - 1e-9
UNDERFLOW_REFUSED = r"scan = (sweep|colour): the acceptance ratio f\^4 of rung 0 underflows to 0 at p=\S+ \(f = \(p / 3\) / \(1 - p\); every p >= 1e-80 is served"
WAVE_REFUSED = r"scan = wave: L=\d+ Nc=\d+ p=\S+ is outside what it is built for"
_A075 = dict(flags=COIN, weaker=dict(swaps=ALL_ACCEPTED_075))
_ANEAR = dict(flags=NEAR, weaker=dict(swaps=ALL_ACCEPTED_NEAR))
_ANEIGH = dict(flags=ON, weaker=dict(swaps=ALL_ACCEPTED_NEIGHBOUR))

ROWS = [
    # ---------------------------------------------------------------------------------------------- A: coinciding and nearly coinciding rungs
    _r("A random toric L3 Nc2 p=.75", "A", "pteq", "toric", 3, 2, 4, 200, 10, "random", 11, 0.75, **_A075),
    _r("A random toric L5 Nc3 p=.75 ragged", "A", "pteq", "toric", 5, 3, 70, 100, 10, "random", 12, 0.75, **_A075),
    _r("A random toric L5 Nc8 p=.75", "A", "pteq", "toric", 5, 8, 5, 200, 10, "random", 13, 0.75, **_A075),
    _r("A random toric L3 Nc12 p=.75", "A", "pteq", "toric", 3, 12, 3, 100, 10, "random", 14, 0.75, **_A075),
    _r("A sweep toric L5 Nc3 p=.75", "A", "pteq", "toric", 5, 3, 5, 200, 10, "sweep", 15, 0.75, **_A075),
    _r("A sweep toric L3 Nc8 p=.75", "A", "pteq", "toric", 3, 8, 4, 200, 10, "sweep", 16, 0.75, **_A075),
    _r("A colour toric L5 Nc2 p=.75", "A", "pteq", "toric", 5, 2, 4, 100, 10, "colour", 17, 0.75, **_A075),
    _r("A colour toric L3 Nc8 p=.75", "A", "pteq", "toric", 3, 8, 3, 100, 10, "colour", 18, 0.75, **_A075),
    _r("A random xzzx L5 Nc3 p=.75", "A", "pteq", "xzzx", 5, 3, 5, 200, 10, "random", 19, 0.75, **_A075),
    _r("A sweep xzzx L3 Nc2 p=.75", "A", "pteq", "xzzx", 3, 2, 4, 200, 10, "sweep", 20, 0.75, **_A075),
    _r("A colour xzzx L5 Nc8 p=.75", "A", "pteq", "xzzx", 5, 8, 3, 100, 10, "colour", 21, 0.75, **_A075),
    _r("A stats random toric L5 Nc3 p=.75", "A", "pteq_stats", "toric", 5, 3, 5, 200, 10, "random", 22, 0.75, **_A075),
    _r("A stats colour toric L3 Nc3 p=.75", "A", "pteq_stats", "toric", 3, 3, 3, 100, 10, "colour", 23, 0.75, **_A075),
    _r("A step toric L5 Nc2 p=.75", "A", "step", "toric", 5, 2, 4, 200, 10, "random", 24, 0.75, **_A075),
    _r("A step xzzx L3 Nc8 p=.75", "A", "step", "xzzx", 3, 8, 4, 200, 10, "random", 25, 0.75, **_A075),
    _r("A random toric L5 Nc2 near", "A", "pteq", "toric", 5, 2, 70, 100, 10, "random", 26, P_NEAR, **_ANEAR),
    _r("A sweep toric L5 Nc2 near", "A", "pteq", "toric", 5, 2, 5, 200, 10, "sweep", 27, P_NEAR, **_ANEAR),
    _r("A colour toric L5 Nc2 near", "A", "pteq", "toric", 5, 2, 4, 100, 10, "colour", 28, P_NEAR, **_ANEAR),
    _r("A random xzzx L5 Nc2 near", "A", "pteq", "xzzx", 5, 2, 5, 200, 10, "random", 29, P_NEAR, **_ANEAR),
    _r("A step toric L3 Nc2 near", "A", "step", "toric", 3, 2, 4, 200, 10, "random", 30, P_NEAR, **_ANEAR),
    _r("A stats random toric L5 Nc2 near", "A", "pteq_stats", "toric", 5, 2, 5, 200, 10, "random", 31, P_NEAR, **_ANEAR),
    _r("A random toric L5 Nc2 neighbour", "A", "pteq", "toric", 5, 2, 70, 100, 10, "random", 32, P_NEIGHBOUR, **_ANEIGH),
    _r("A sweep toric L5 Nc2 neighbour", "A", "pteq", "toric", 5, 2, 5, 200, 10, "sweep", 33, P_NEIGHBOUR, **_ANEIGH),
    _r("A colour toric L5 Nc2 neighbour", "A", "pteq", "toric", 5, 2, 4, 100, 10, "colour", 34, P_NEIGHBOUR, **_ANEIGH),
    _r("A wave toric L5 Nc2 neighbour", "A", "pteq", "toric", 5, 2, 70, 100, 10, "wave", 35, P_NEIGHBOUR, flags=ON),       # (one refusal in 7 000 tests)
    _r("A wave toric L5 Nc2 p=.75 refused", "A", "pteq", "toric", 5, 2, 4, 100, 10, "wave", 36, 0.75, refusal=WAVE_REFUSED),
    _r("A wave toric L5 Nc8 p=.75 refused", "A", "pteq", "toric", 5, 8, 4, 100, 10, "wave", 37, 0.75, refusal=WAVE_REFUSED),
    _r("A wave xzzx L5 Nc3 p=.75 refused", "A", "pteq", "xzzx", 5, 3, 4, 100, 10, "wave", 38, 0.75, refusal=WAVE_REFUSED),
    _r("A wave toric L5 Nc2 near refused", "A", "pteq", "toric", 5, 2, 4, 100, 10, "wave", 39, P_NEAR, refusal=WAVE_REFUSED),
    # ---------------------------------------------------------------------------------------------- B: each side of the single-precision bound
    _r("B alpha mixed random", "B", "pteq", "rotated", 5, 4, 5, 200, 10, "random", 41, 0.01, alpha=8.0, flags=TABLE, f32="mixed", weaker=dict(proposals=ALPHA_TOP)),
    _r("B alpha mixed random ragged", "B", "pteq", "xzzx", 3, 4, 70, 100, 10, "random", 42, 0.01, alpha=8.0, flags=TABLE, f32="mixed", weaker=dict(proposals=ALPHA_TOP)),
    _r("B alpha mixed step", "B", "step", "rotated", 5, 4, 4, 200, 10, "random", 43, 0.01, alpha=8.0, flags=TABLE, f32="mixed", weaker=dict(proposals=ALPHA_TOP)),
    _r("B alpha mixed colour", "B", "pteq", "rotated", 5, 4, 6, 300, 10, "colour", 44, 0.01, alpha=8.0, flags=COLOUR_ALPHA, f32="mixed"),
    _r("B alpha on random", "B", "pteq", "rotated", 5, 4, 5, 200, 10, "random", 45, 0.01, alpha=6.0, flags=TABLE, f32="on", weaker=dict(proposals=ALPHA_TOP)),
    _r("B alpha on colour", "B", "pteq", "rotated", 5, 4, 6, 300, 10, "colour", 46, 0.01, alpha=6.0, flags=COLOUR_ALPHA, f32="on"),
    _r("B alpha on wave", "B", "pteq", "rotated", 5, 4, 5, 200, 10, "wave", 47, 0.01, alpha=6.0, flags=TABLE, f32="on"),
    _r("B alpha iters 600 random", "B", "pteq", "xzzx", 3, 4, 3, 100, 600, "random", 48, 0.1, alpha=2.0, flags=TABLE, f32="off", weaker=dict(proposals=ALPHA_TOP)),
    _r("B alpha iters 600 step", "B", "step", "xzzx", 3, 4, 3, 100, 600, "random", 49, 0.1, alpha=2.0, flags=TABLE, f32="off", weaker=dict(proposals=ALPHA_TOP)),
    _r("B alpha iters 512 random", "B", "pteq", "xzzx", 3, 4, 3, 100, 512, "random", 50, 0.8, alpha=2.0, flags=TABLE, f32="on", weaker=dict(proposals=ALPHA_TOP)),
    _r("B alpha iters 513 random", "B", "pteq", "xzzx", 3, 4, 3, 100, 513, "random", 51, 0.8, alpha=2.0, flags=TABLE, f32="off", weaker=dict(proposals=ALPHA_TOP)),
    _r("B biased on random", "B", "pteq", "xzzx", 5, 4, 5, 200, 10, "random", 52, 0.1, eta=1e6, flags=TABLE, f32="on"),
    _r("B biased off random", "B", "pteq", "xzzx", 5, 4, 5, 200, 25, "random", 53, 0.1, eta=1e6, flags=TABLE, f32="off"),
    _r("B biased off random ragged", "B", "pteq", "rotated", 3, 5, 70, 100, 25, "random", 54, 0.1, eta=1e6, flags=TABLE, f32="off"),
    _r("B biased off step", "B", "step", "xzzx", 5, 4, 4, 200, 25, "random", 55, 0.1, eta=1e6, flags=TABLE, f32="off"),
    _r("B biased on colour", "B", "pteq", "xzzx", 5, 4, 3, 100, 10, "colour", 56, 0.1, eta=1e6, flags=TABLE, f32="on"),
    _r("B biased off colour", "B", "pteq", "xzzx", 5, 4, 3, 100, 25, "colour", 57, 0.1, eta=1e6, flags=TABLE, f32="off"),
    _r("B alpha uset on", "B", "ptdc", "xzzx", 5, 1, 3, 200, 5, "random", 58, 0.01, alpha=8.0, flags=TABLE, f32="on"),
    _r("B alpha uset off", "B", "ptdc", "xzzx", 5, 1, 3, 200, 10, "random", 59, 0.01, alpha=8.0, flags=TABLE, f32="off"),
    _r("B alpha mixed wave refused", "B", "pteq", "rotated", 5, 4, 4, 100, 10, "wave", 60, 0.01, alpha=8.0, refusal=WAVE_REFUSED),
    _r("B alpha iters 600 wave refused", "B", "pteq", "xzzx", 3, 4, 4, 100, 600, "wave", 61, 0.1, alpha=2.0, refusal=WAVE_REFUSED),
]


def _low(p, tag, sat, seed0, underflow=False):
    """group C at one p: the three table-free scans, and scan = wave in both cascade forms at 2, 5 and 8 rungs.  underflow: f^4 is 0 in double precision, which
    the sweep and colour kernels' x <= threshold - 1 cannot say -- refused by name (csrc/plan_host.hpp), found by these rows"""
    table = dict(refusal=UNDERFLOW_REFUSED) if underflow else dict(flags=ON, sat=sat)
    return [
        _r("C random toric L5 Nc5 " + tag, "C", "pteq", "toric", 5, 5, 5, 200, 10, "random", seed0, p, flags=ON, sat=sat),
        _r("C sweep xzzx L5 Nc4 " + tag, "C", "pteq", "xzzx", 5, 4, 5, 200, 10, "sweep", seed0 + 1, p, **table),
        _r("C colour toric L3 Nc4 " + tag, "C", "pteq", "toric", 3, 4, 3, 100, 10, "colour", seed0 + 2, p, **table),
        _r("C wave toric L5 Nc5 " + tag, "C", "pteq", "toric", 5, 5, 70, 100, 10, "wave", seed0 + 3, p, flags=ON, sat=sat),
        _r("C wave toric L3 Nc2 " + tag, "C", "pteq", "toric", 3, 2, 70, 200, 10, "wave", seed0 + 4, p, flags=ON, sat=sat),
        _r("C wave rotated L5 Nc8 " + tag, "C", "pteq", "rotated", 5, 8, 5, 200, 10, "wave", seed0 + 5, p, flags=ON, sat=sat),
    ]


ROWS += (_low("thr32", "p=thr32", "thr32", 100) + _low("thr44", "p=thr44", "thr44", 110) + _low(1e-3, "p=1e-3", "thr32", 120) + _low(1e-6, "p=1e-6", "thr44", 130)
         + _low(1e-12, "p=1e-12", "thr44", 140) + _low(1e-300, "p=1e-300", "underflow", 190, True) + _low("min", "p=min", "zero", 160, True))
ROWS += [
    # the last decade the sweep and colour kernels serve: f^4 = 1.2e-322 is still a number
    _r("C sweep xzzx L5 Nc4 p=1e-80", "C", "pteq", "xzzx", 5, 4, 5, 200, 10, "sweep", 166, 1e-80, flags=ON, sat="thr44"),
    _r("C sweep toric L5 Nc4 p=1e-80", "C", "pteq", "toric", 5, 4, 5, 200, 10, "sweep", 167, 1e-80, flags=ON, sat="thr44"),
    _r("C colour toric L3 Nc4 p=1e-80", "C", "pteq", "toric", 3, 4, 3, 100, 10, "colour", 168, 1e-80, flags=ON, sat="thr44"),
    _r("C wave config 2 p=1e-6", "C", "pteq", "toric", 9, 8, 70, 100, 10, "wave", 170, 1e-6, flags=ON, sat="thr44"),
    _r("C wave toric L5 Nc9 p=1e-6", "C", "pteq", "toric", 5, 9, 4, 200, 10, "wave", 171, 1e-6, flags=ON, sat="thr44"),
    _r("C random toric L3 Nc12 p=1e-6", "C", "pteq", "toric", 3, 12, 3, 200, 10, "random", 172, 1e-6, flags=ON, sat="thr44"),
    _r("C random toric L5 Nc8 p=1e-6 ragged", "C", "pteq", "toric", 5, 8, 70, 100, 10, "random", 173, 1e-6, flags=ON, sat="thr44"),
    _r("C stats random toric L5 Nc4 p=1e-6", "C", "pteq_stats", "toric", 5, 4, 5, 200, 10, "random", 174, 1e-6, flags=ON, sat="thr44"),
    _r("C stats wave toric L5 Nc4 p=1e-300", "C", "pteq_stats", "toric", 5, 4, 5, 200, 10, "wave", 175, 1e-300, flags=ON, sat="underflow", forms=(0,)),
    _r("C step toric L5 Nc4 p=1e-12", "C", "step", "toric", 5, 4, 4, 200, 10, "random", 176, 1e-12, flags=ON, sat="thr44"),
    _r("C chain toric L5 p=1e-6", "C", "chain", "toric", 5, 1, 6, 1, 300, "random", 177, 1e-6, flags=dict(swap_fast_ok=1, top_acc=0, lower_acc=0), sat="thr44"),
    _r("C chain xzzx L5 p=min", "C", "chain", "xzzx", 5, 1, 6, 1, 300, "random", 178, "min", flags=dict(swap_fast_ok=1, top_acc=0, lower_acc=0), sat="zero"),
    # the criterion (SEQ = 2, TOPS = 5, eps = 0.1, tops_burn = 1) under a cap of 300 steps: the flag comes back so rarely that most ladders run into the cap
    _r("C criterion toric L3 Nc5 p=1e-3", "C", "pteq_conv", "toric", 3, 5, 70, 300, 10, "random", 179, 1e-3, flags=ON, sat="thr32", crit=dict(SEQ=2, TOPS=5, eps=0.1)),
    _r("C biased xzzx L5 Nc4 p=1e-6", "C", "pteq", "xzzx", 5, 4, 5, 200, 10, "random", 180, 1e-6, eta=100.0, flags=TABLE, f32="on"),
    _r("C alpha xzzx L5 Nc4 pz=1e-6", "C", "pteq", "xzzx", 5, 4, 5, 200, 10, "random", 181, 1e-6, alpha=2.0, flags=TABLE, f32="on"),
]
ROW = {r["id"]: r for r in ROWS}
assert len(ROW) == len(ROWS)


# ------------------------------------------------------------------------------------------------------------------ the plan, read on the host
def noise_of(row):
    return L_.NOISE_ALPHA if row["alpha"] else L_.NOISE_BIASED if row["eta"] else L_.NOISE_DEPOLARIZING


def make_block(code, L, Nc, p, scan="random", iters=10, eta=None, alpha=None, p_logical=0.5, **kw):
    return L_.make_params(code=CODES.index(code), L=L, Nc=Nc, p=p, p_logical=p_logical, iters=iters, scan=SCANS.index(scan),
                          noise=L_.NOISE_ALPHA if alpha else L_.NOISE_BIASED if eta else L_.NOISE_DEPOLARIZING, eta=eta or 0.0, alpha=alpha or 0.0, **kw)


def read_plan(pr, Nc):
    """validate_params() and plan_host() on a parameter block (qt_plan_ladder, csrc/tables_test_api.cpp): rc, msg, and of an accepted block the ladder's
    flags -- top_acc, lower_acc, swap_fast_ok, the per-rung bias_f32ok bits -- and its tables: acc_thr / acc_thr44 [Nc][4], acc_top[nq + 1],
    swap_thr[Nc - 1][nq + 1], swap_inv_log2[Nc - 1]"""
    T = tables_lib()
    T.qt_plan_ladder.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    head, inv, thr, thr44 = np.zeros(4, np.uint32), np.zeros(16, np.float32), np.zeros((16, 4), np.uint32), np.zeros((16, 4), np.uint64)
    top, swap, msg = np.zeros(2 * 64 * 64 + 1, np.uint32), np.zeros(16 * (2 * 64 * 64 + 1), np.uint64), C.create_string_buffer(700)
    rc = T.qt_plan_ladder(C.byref(pr), head.ctypes.data, inv.ctypes.data, thr.ctypes.data, thr44.ctypes.data, top.ctypes.data, top.size, swap.ctypes.data,
                          swap.size, msg, len(msg))
    out = dict(rc=rc, msg=msg.value.decode())
    if rc == 0:
        mask, nq = int(head[0]), int(head[3])
        out.update(top_acc=mask >> (Nc - 1) & 1, lower_acc=int(mask & ((1 << (Nc - 1)) - 1) != 0), swap_fast_ok=int(head[1]), nq=nq,
                   f32=[int(head[2]) >> c & 1 for c in range(Nc)], acc_thr=thr[:Nc].copy(), acc_thr44=thr44[:Nc].copy(), acc_top=top[:nq + 1].copy(),
                   swap_thr=swap[:(Nc - 1) * (nq + 1)].reshape(Nc - 1, nq + 1).copy(), swap_inv_log2=inv[:max(Nc - 1, 0)].copy())
    return out


@functools.lru_cache(maxsize=None)
def edge_p(which):
    """the largest p at which ceil(f^4 2^32) == 1 ("thr32") / ceil(f^4 2^44) == 1 ("thr44"), f = (p / 3) / (1 - p): bisection over the doubles on the bottom
    rung's entry of a plan's own table (acc_thr / acc_thr44 [0][3]); both ends are asserted in tests/test_sampler_range_cpu.py"""
    key = dict(thr32="acc_thr", thr44="acc_thr44")[which]
    at = lambda p: int(read_plan(make_block("toric", 3, 2, p), 2)[key][0][3])
    lo, hi = 1e-4, 0.05
    assert at(lo) == 1 < at(hi)
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            return lo
        lo, hi = (mid, hi) if at(mid) == 1 else (lo, mid)


def p_of(row):
    p = row["p"]
    return MIN_DOUBLE if p == "min" else edge_p(p) if isinstance(p, str) else p


def block_of(row, flags=0):
    """the parameter block the row's entry point hands the library"""
    if row["entry"] in ("ptdc", "chain"):          # (ptdc_batch: a ladder without logical moves; a single chain has no plan -- its tables are those of one rung)
        return make_block(row["code"], row["L"], row["Nc"], p_of(row), iters=row["iters"], eta=row["eta"], alpha=row["alpha"], p_logical=0.0)
    return make_block(row["code"], row["L"], row["Nc"], p_of(row), row["scan"], row["iters"], row["eta"], row["alpha"], steps=row["steps"],
                      first_syndrome=row["first_syndrome"], flags=flags)


def plan_of(row):
    return read_plan(block_of(row), row["Nc"])


def f32_name(bits):
    """"on" / "off" of the rungs below the top (what the kernels' choice reads), "mixed": the hot ones on and the cold ones off"""
    lower = bits[:-1] if len(bits) > 1 else bits
    if all(lower) or not any(lower):
        return "on" if all(lower) else "off"
    k = lower.index(1)
    return "mixed" if all(lower[k:]) else "mixed, not monotone"


# ------------------------------------------------------------------------------------------------------------------ inputs
def state_shape(row):
    L = row["L"]
    return (2, L, L) if row["code"] in ("toric", "planar") else (L, L)


def class_reps(orc, row, m):
    if row["code"] == "toric":
        return np.stack([np.stack([orc.toric_to_class(x, e) for e in range(16)]) for x in m])
    ocode = getattr(orc, row["code"].upper())
    return np.stack([np.stack([orc.surf_apply_logical(ocode, x, op)[0] for op in range(4)]) for x in m])


def make_init(row):
    """the seeds of the batch, drawn from the row's seed at density P_INIT whatever the sampling p (ptdc: one representative per class and syndrome)"""
    rng = np.random.default_rng(row["seed"])
    shape = (row["N"],) + state_shape(row)
    m = np.zeros(shape, np.uint8)
    err = rng.random(shape) < P_INIT
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    if row["entry"] == "ptdc":
        from oracle import oracle as orc
        m = class_reps(orc, row, m)
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------------------------------------------------------ the oracle
def _rule(row, for_oracle):
    if row["alpha"]:
        return dict(noise=2, alpha=row["alpha"], det_pow=1) if for_oracle else dict(alpha=row["alpha"])
    if row["eta"]:
        return dict(noise=1, eta=row["eta"]) if for_oracle else dict(eta=row["eta"])
    return {}


def class_of(orc, row, m):
    return orc.toric_eq_class(m) if row["code"] == "toric" else orc.surf_eq_class(getattr(orc, row["code"].upper()), m)


def stepped(orc, row, init, ladders=None):
    """the oracle's ladders stepped from Python: final states, flags, tops0, (n_z, n_x + n_y) under the alpha rule, swap_accepts and nerr_sums of every
    ladder, and the first step with tops0 >= TOPS (0: none)"""
    ocode, scan, p = getattr(orc, row["code"].upper()), SCANS.index(row["scan"]), p_of(row)
    out = dict(states=[], flags=[], tops0=[], neff=[], swap_accepts=[], nerr_sums=[], reached=[])
    for l in (range(row["N"]) if ladders is None else ladders):
        ld = orc.Ladder(ocode, init[l], p, row["Nc"], 0.5, scan=scan, **_rule(row, True))
        rng, reached = orc.Rng.philox(row["seed"], row["first_syndrome"] + l), 0
        for t in range(row["steps"]):
            ld.step(row["iters"], rng)
            if not reached and ld.tops0 >= TOPS:
                reached = t + 1
        out["states"].append(ld.states); out["flags"].append(ld.flags); out["tops0"].append(ld.tops0); out["reached"].append(reached)
        out["swap_accepts"].append(ld.swap_accepts); out["nerr_sums"].append(ld.nerr_sums)
        if row["alpha"]:
            out["neff"].append(ld.n_eff_counts)
    return {k: np.array(v) for k, v in out.items()}


DIAG_STREAM = 0x400                        # a ladder's rung c below the top draws step T's proposals from stream DIAG_STREAM + (c + T) mod Nc (DESIGN.md "RNG addressing")


def chain_step(orc, row, m, c, p_c, k0, iters, rng, step=None):
    """`iters` proposals of a chain at p_c from proposal k0 (Chain.update_chain); step = T: as rung c of a ladder runs them in its step T"""
    top = step is not None and c == row["Nc"] - 1
    ocode, pl, slot = getattr(orc, row["code"].upper()), 0.5 if top else 0.0, c if top or step is None else DIAG_STREAM + (c + step) % row["Nc"]
    if row["alpha"]:
        return orc.chain_update_alpha(ocode, m, p_c, row["alpha"], pl, iters, rng, slot=slot, k0=k0)[0]
    if row["eta"]:
        return orc.chain_update(ocode, m, p_c, pl, iters, rng, slot=slot, k0=k0, noise=orc.BIASED, eta=row["eta"])
    return orc.chain_update(ocode, m, p_c, pl, iters, rng, slot=slot, k0=k0)


def proposal_witness(orc, row, init, ladder=0):
    """[accepted, rejected] per rung of one ladder: the ladder stepped from Python, every rung's proposals of a step replayed as single chains of 1, 2, ... proposals
    from the state the step began with (a proposal was accepted iff it changed the state) -- until every rung has shown both.  The replay is
    held to the ladder: after a step's proposals the rungs' states are the ladder's, up to the order the swaps leave them in."""
    ocode, p, Nc, iters = getattr(orc, row["code"].upper()), p_of(row), row["Nc"], row["iters"]
    ld = orc.Ladder(ocode, init[ladder], p, Nc, 0.5, scan=0, **_rule(row, True))
    stream = row["first_syndrome"] + ladder
    rng, seen = orc.Rng.philox(row["seed"], stream), np.zeros((Nc, 2), bool)
    pl = ld.p_ladder
    for t in range(row["steps"]):
        before = ld.states
        ld.step(iters, rng)
        after = sorted(s.tobytes() for s in ld.states)
        ends = []
        for c in range(Nc):
            # (prefixes of the step's own call: the table-driven rules freeze the weight of the state a call begins with, so j calls of one proposal are
            # another chain)
            m, whole = before[c], lambda j: chain_step(orc, row, before[c], c, pl[c], t * iters, j, orc.Rng.philox(row["seed"], stream), step=t)
            for j in range(1, iters + 1):
                if seen[c].all():
                    break
                n = whole(j)
                seen[c, 0 if (n != m).any() else 1] = True
                m = n
            ends.append(whole(iters))
        assert sorted(e.tobytes() for e in ends) == after, "the single-chain replay left the ladder's trajectory at step %d" % t
        if seen.all():
            break
    return seen


def run_oracle(orc, row, init):
    """everything the row's entry point returns, from the oracle on the same Philox streams"""
    ocode, scan, p = getattr(orc, row["code"].upper()), SCANS.index(row["scan"]), p_of(row)
    common = dict(iters=row["iters"], seed=row["seed"], first_syndrome=row["first_syndrome"])
    if row["entry"] == "ptdc":
        hist, mh, xv = orc.ptdc_batch(ocode, init, p, row["Nc"], row["steps"], with_m=True, with_xyz=True, alpha=row["alpha"], **common)
        from qecmc.decoders import unpack_xyz          # (sorted, as ptdc_batch returns the sets)
        return dict(hist=hist, mhist=mh, xyz=[[unpack_xyz(xv[s, c]) for c in range(xv.shape[1])] for s in range(xv.shape[0])])
    if row["entry"] == "chain":
        return dict(states=np.stack([chain_step(orc, row, init[i], 0, p, 0, row["iters"], orc.Rng.philox(row["seed"], row["first_syndrome"] + i))
                                     for i in range(row["N"])]))
    if row["entry"] == "pteq_conv":
        return orc.pteq_batch(ocode, init, p, row["Nc"], row["steps"], tops_burn=CONV_TOPS_BURN, conv_criteria="error_based", scan=scan, **row["crit"], **_rule(row, True), **common)
    st = stepped(orc, row, init)
    if row["entry"] == "step":
        return st
    ref = orc.pteq_batch(ocode, init, p, row["Nc"], row["steps"], tops_burn=0, return_states=True, scan=scan, **_rule(row, True), **common)
    assert np.array_equal(ref["states"], st["states"]) and np.array_equal(ref["tops0"], st["tops0"]), "the oracle's batch and its ladders stepped from Python differ"
    ref.update(swap_accepts=st["swap_accepts"], nerr_sums=st["nerr_sums"], flags=st["flags"])
    if row["scan"] == "colour":          # (a fixed-length run of scan = colour reports the first step with tops0 >= TOPS, tests/test_gpu_colour.py)
        ref["steps_done"], ref["converged"] = np.where(st["reached"] > 0, st["reached"], row["steps"]), st["reached"] > 0
    return ref


def vacuous(orc, row, init, ref):
    """why the oracle's run of the row would prove nothing -- [] when it proves something.  Conditions on the reference alone; where row["weaker"] names
    one, the weaker statement it gives is held instead"""
    why, N, Nc, weaker = [], row["N"], row["Nc"], row["weaker"]
    if row["entry"] == "ptdc":
        if not (ref["hist"].reshape(-1, ref["hist"].shape[-1]).sum(axis=1) >= 2).all():
            why.append("a set holds fewer than two distinct configurations")
        return why
    if row["entry"] == "pteq_conv":
        capped = (ref["steps_done"] == row["steps"]) & ~ref["converged"]
        if not (capped & (np.asarray(ref["samples"]) > 0)).any():
            why.append("no ladder runs into the step cap with samples booked")
        if not (ref["converged"] & (ref["steps_done"] < row["steps"])).any():
            why.append("no ladder stops before the cap")
        return why
    states = ref["states"].reshape(N, Nc, -1) if row["entry"] != "chain" else ref["states"].reshape(N, 1, -1)
    moved = (states != np.asarray(init).reshape(N, 1, -1)).any(axis=2)
    if not (2 * moved.sum(axis=0) > N).all():
        why.append("a rung ends where it started in half of the ladders or more: %r of %d ladders moved, per rung" % (moved.sum(axis=0).tolist(), N))
    if row["entry"] == "chain":
        return why
    acc, tests = ref["swap_accepts"].sum(axis=0), N * row["steps"]
    if "swaps" in weaker:
        if not (acc == tests).all():
            why.append("a swap is refused where every swap should be accepted (%s)" % weaker["swaps"])
    elif Nc > 1 and not ((acc > 0) & (acc < tests)).all():
        why.append("a pair without an accepted or without a refused swap: accepted %r of %d" % (acc.tolist(), tests))
    if row["group"] == "B" and row["scan"] == "random":
        seen = np.zeros((Nc, 2), bool)
        for l in range(min(N, 4)):          # (the first ladders of the batch, until every rung has shown both)
            seen |= proposal_witness(orc, row, init, l) if not seen.all() else seen
        if "proposals" in weaker:          # (the top rung: nothing is said of rejections -- a logical move at the identity position leaves the state as it is)
            seen[Nc - 1, 1] = True
        if not seen.all():
            why.append("[accepted, rejected] proposals seen per rung: %r" % seen.tolist())
    return why


# ------------------------------------------------------------------------------------------------------------------ the library
def fresh(row, init):
    """Ladder.__init__: every rung holds init, the flag on the top rung; (n_z, n_x + n_y) per rung for the alpha rule"""
    n, Nc = len(init), row["Nc"]
    states = np.array(np.broadcast_to(np.asarray(init).reshape(n, 1, -1), (n, Nc, init[0].size)), order="C")
    flags = np.zeros((n, Nc), np.uint8); flags[:, -1] = 1
    neff = np.ascontiguousarray(np.stack([(states == 3).sum(axis=2), ((states == 1) | (states == 2)).sum(axis=2)], axis=2).astype(np.uint16))
    return states, flags, neff


def run_gpu(q, row, init, flags=0):
    """the row's call; raises QecmcError where the library refuses it"""
    code, p, N = getattr(q, row["code"].upper()), p_of(row), row["N"]
    common = dict(Nc=row["Nc"], steps=row["steps"], iters=row["iters"], seed=row["seed"], first_syndrome=row["first_syndrome"], code=code)
    if row["entry"] == "ptdc":
        hist, mh, xyz = q.ptdc_batch(np.array(init), p, with_m=True, with_xyz=True, alpha=row["alpha"], **common)
        return dict(hist=hist, mhist=mh, xyz=xyz)
    if row["entry"] == "chain":
        m = np.array(init)
        L_.check(L_.lib().qecmc_chain_update(CODES.index(row["code"]), row["L"], N, L_.u8(m), float(p), 0.0, row["iters"], row["seed"], row["first_syndrome"], 0, 0))
        return dict(states=m)
    if row["entry"] == "step":
        states, fl, neff = fresh(row, init)
        tops0, pr = np.zeros(N, np.uint32), block_of(row)
        pr.seed = row["seed"]
        if row["alpha"]:
            L_.check(L_.lib().qecmc_ladder_step_alpha(pr, N, L_.u8(states), L_.u8(fl), L_.u32(tops0), L_.u16(neff), row["iters"], row["steps"], 0, 0))
        else:
            L_.check(L_.lib().qecmc_ladder_step(pr, N, L_.u8(states), L_.u8(fl), L_.u32(tops0), row["iters"], row["steps"], 0, 0))
        out = dict(states=states.reshape((N, row["Nc"]) + init.shape[1:]), flags=fl, tops0=tops0)
        if row["alpha"]:
            out["neff"] = neff
        return out
    if row["entry"] == "pteq_conv":
        return q.pteq_batch(np.array(init), p, tops_burn=CONV_TOPS_BURN, scan=row["scan"], conv_criteria="error_based", flags=flags, **row["crit"], **_rule(row, False), **common)
    return q.pteq_batch(np.array(init), p, tops_burn=0, scan=row["scan"], flags=flags, return_states=row["entry"] == "pteq",
                        return_swap_stats=row["entry"] == "pteq_stats", **_rule(row, False), **common)


def differences(row, got, ref):
    """the returned fields in which the library's answer differs from the oracle's, bit for bit"""
    same = lambda k: np.array_equal(np.asarray(got[k]).astype(np.uint64), np.asarray(ref[k]).astype(np.uint64))
    if row["entry"] == "ptdc":
        bad = [k for k in ("hist", "mhist") if not np.array_equal(got[k], ref[k])]
        if not all(len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b)) for a, b in zip(got["xyz"], ref["xyz"])):
            bad.append("xyz")
        return bad
    if row["entry"] == "chain":
        return [] if np.array_equal(got["states"], ref["states"]) else ["states"]
    if row["entry"] == "step":
        return [k for k in ("states", "flags", "tops0") + (("neff",) if row["alpha"] else ()) if not same(k)]
    keys = ["counts", "samples", "tops0", "steps_done", "converged"]
    keys += dict(pteq=["states"], pteq_stats=["swap_accepts", "nerr_sums"], pteq_conv=[])[row["entry"]]
    return [k for k in keys if not same(k)]
