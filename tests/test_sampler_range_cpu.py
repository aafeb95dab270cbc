"""The samplers at the ends of their parameter range, the half that needs no GPU (tests/range_cases.py is the table; tests/test_gpu_sampler_range.py runs the
kernels).  For every row:

  (a) the plan presents what the row is there for -- swap_fast_ok, top_acc, lower_acc and the per-rung bias_f32ok mask, read from plan_host() through the
      host test API (qt_plan_ladder), or the refusal by name -- and the flag tuple is one the sweep of tests/test_kernel_choice.py runs for the rule and scan;
  (b) group C: the tables have saturated the way the row says -- thresholds of 1 (of 0 where the factor underflows), flat swap rows, swap_inv_log2 = 0
      exactly where log2 p_diff is not finite -- and wu_swap_bound() still equals the brute-force maximum on those rows;
  (c) the oracle's run alone is not vacuous (range_cases.vacuous): every rung leaves its start, every pair of rungs shows an accepted and a refused swap,
      every rung of group B an accepted and a rejected proposal -- or the weaker statement the row records with its reason;
  (d) the oracle is deterministic at p = 1e-300 and at the smallest positive double.

Run with -s, every test prints the flags, the saturation and the bisected bounds it found."""
import ctypes as C
import math

import numpy as np
import pytest

import range_cases as R
from hostlib import tables_lib
from test_kernel_choice import ladders

ROWS = R.ROWS
IDS = [r["id"] for r in ROWS]


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_wave_swap_bound.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_plan_presents_the_premise(row):
    plan = R.plan_of(row)
    if "refusal" in row:
        assert plan["rc"] == -4 and __import__("re").search(row["refusal"], plan["msg"]), plan
        print("%-44s refused: %s" % (row["id"], plan["msg"][:90]))
        return
    assert plan["rc"] == 0, plan["msg"]
    got = {k: plan[k] for k in ("swap_fast_ok", "top_acc", "lower_acc")}
    print("%-44s p=%-24r %s f32ok=%s" % (row["id"], R.p_of(row), got, plan["f32"]))
    assert got == row["flags"]
    if "f32" in row:
        assert R.f32_name(plan["f32"]) == row["f32"], plan["f32"]
    # the tuple is one the CPU sweep of the kernel choice runs for this rule and scan (test_kernel_choice.ladders): what is run here is chosen there
    lower = plan["f32"][:-1]
    tup = (got["top_acc"], got["lower_acc"], got["swap_fast_ok"], int(all(lower)))
    assert tup in ladders(R.noise_of(row), R.SCANS.index(row["scan"]), row["Nc"]), tup


def test_both_sides_of_every_premise_are_in_the_table():
    """swap_fast_ok on and off (off with lower_acc on and off), bias_f32ok on / mixed / off under both rules' entry points, every saturation of group C --
    each with a row that runs (the refusals beside them)"""
    run = [r for r in ROWS if "refusal" not in r]
    assert {(r["flags"]["swap_fast_ok"], r["flags"]["lower_acc"]) for r in run if r["group"] == "A"} == {(0, 1), (0, 0), (1, 0)}
    assert {r["f32"] for r in run if r["alpha"]} == {"on", "mixed", "off"} and {r["f32"] for r in run if r["eta"]} == {"on", "off"}
    assert {r["sat"] for r in run if r["group"] == "C" and "sat" in r} == {"thr32", "thr44", "underflow", "zero"}
    for scan in R.SCANS[:3]:
        assert any(r["scan"] == scan and r["flags"]["swap_fast_ok"] == 0 for r in run)
    assert {r["entry"] for r in run} == {"pteq", "pteq_stats", "pteq_conv", "step", "chain", "ptdc"}
    assert {(r["scan"], r["refusal"]) for r in ROWS if "refusal" in r} == {("wave", R.WAVE_REFUSED), ("sweep", R.UNDERFLOW_REFUSED), ("colour", R.UNDERFLOW_REFUSED)}


def test_near_coincidence_is_decided_by_the_plan():
    """the p just below 0.75 of group A: at P_NEAR a threshold of d = 1 has left 32 bits while the rungs still differ, at P_NEIGHBOUR it has not"""
    near, neigh = (R.read_plan(R.make_block("toric", 5, 2, p), 2) for p in (R.P_NEAR, R.P_NEIGHBOUR))
    assert near["swap_thr"][0, 1] == 1 << 32 and near["swap_fast_ok"] == 0 and near["lower_acc"] == 0 and near["acc_thr44"][0, 0] < 1 << 44
    assert neigh["swap_thr"][0, 1] < 1 << 32 and neigh["swap_fast_ok"] == 1
    print("swap_thr[0][1]: %d at 0.75 - 1e-11, %d at 0.75 - 1e-9" % (near["swap_thr"][0, 1], neigh["swap_thr"][0, 1]))


# ---------------------------------------------------------------------------------------------------------------- (b)
def test_bisected_bounds():
    """the largest p whose ceil(f^4 2^32) / ceil(f^4 2^44) is 1: f^4 <= 2^-32 at f = 2^-8, p = 3 / 259; f^4 <= 2^-44 at f = 2^-11, p = 3 / 2051"""
    for which, key, exact in (("thr32", "acc_thr", 3 / 259), ("thr44", "acc_thr44", 3 / 2051)):
        p = R.edge_p(which)
        above = math.nextafter(p, 1.0)
        at = lambda x: int(R.read_plan(R.make_block("toric", 3, 2, x), 2)[key][0][3])
        print("%s: p = %r (%s), the table's entry %d there and %d one double above" % (which, p, p.hex(), at(p), at(above)))
        assert at(p) == 1 and at(above) == 2
        assert abs(p - exact) <= 4 * math.ulp(exact)


def test_sweep_and_colour_are_refused_exactly_where_f4_underflows():
    """the smallest p scan = sweep and scan = colour serve: the first double whose f^4 is not 0 (bisection on the plan's answer), below 1e-80 as the message
    promises; one double lower the plan is refused by name, and scan = random / wave still make theirs"""
    rc = lambda p, scan: R.read_plan(R.make_block("toric", 3, 2, p, scan), 2)
    lo, hi = 1e-90, 1e-80
    assert rc(lo, "sweep")["rc"] == -4 and rc(hi, "sweep")["rc"] == 0
    while True:
        mid = math.sqrt(lo) * math.sqrt(hi)
        if not lo < mid < hi:
            break
        lo, hi = (lo, mid) if rc(mid, "sweep")["rc"] == 0 else (mid, hi)
    while math.nextafter(lo, 1.0) < hi:          # (the geometric mean stalls a few doubles apart)
        nxt = math.nextafter(lo, 1.0)
        lo, hi = (lo, nxt) if rc(nxt, "sweep")["rc"] == 0 else (nxt, hi)
    print("scan = sweep / colour serve p >= %r (%s): acc_thr[0] = %s there" % (hi, hi.hex(), rc(hi, "sweep")["acc_thr"][0].tolist()))
    assert hi < 1e-80 and rc(hi, "sweep")["acc_thr"][0][3] == 1
    for scan in ("sweep", "colour"):
        assert rc(hi, scan)["rc"] == 0
        bad = rc(lo, scan)
        assert bad["rc"] == -4 and __import__("re").search(R.UNDERFLOW_REFUSED, bad["msg"]), bad
    for scan in ("random", "wave"):
        ok = rc(lo, scan)
        assert ok["rc"] == 0 and ok["acc_thr"][0][3] == 0 and ok["acc_thr44"][0][3] == 0


def _saturation(row, plan):
    """what the row's `sat` says of the bottom rung's thresholds and of the swap row above it"""
    t32, t44, top, sat = plan["acc_thr"][0], plan["acc_thr44"][0], plan["acc_top"], row["sat"]
    swap = plan["swap_thr"][0] if row["Nc"] > 1 else None
    if sat == "thr32":          # ceil(f^4 2^32) has reached 1, the 44-bit word may still resolve
        assert t32[3] == 1 and t32[0] > 1
    elif sat == "thr44":        # ... and ceil(f^4 2^44)
        assert t32[3] == 1 and t44[3] == 1
    elif sat == "underflow":    # f is a number, f^4 is not: 1, then 0
        assert t32[0] == 1 and t44[0] == 1 and t32[3] == 0 and t44[3] == 0
        assert swap is None or (swap[1] == 1 and (swap[2:] == 0).all())
    else:                       # f = 0: nothing passes (p_diff is 0 beside a top rung, a few times the smallest double beside another: 1, then 0)
        assert (t32 == 0).all() and (t44 == 0).all()
        assert swap is None or (swap[1] == (0 if row["Nc"] == 2 else 1) and (swap[2:] == 0).all())
    if swap is not None and sat != "thr32":
        flat = np.flatnonzero(swap[1:-1] == swap[2:]) + 1
        assert flat.size, "no two neighbouring entries of the bottom pair's swap row are equal"
    for i in range(row["Nc"] - 1):
        # swap_inv_log2 = 1 / log2 p_diff, and 0 exactly where that logarithm is not finite: p_diff read back from the row's own first entry
        dead = plan["swap_thr"][i, 1] == 0
        assert (plan["swap_inv_log2"][i] == 0) == bool(dead), (i, plan["swap_inv_log2"][i], plan["swap_thr"][i, 1])
    assert top[0] == 0 and (top[1:] == 0xFFFFFFFF).all()          # (acc_top serves a top chain below p = 0.75; these ladders' top rung takes the coin)


@pytest.mark.parametrize("row", [r for r in ROWS if r.get("sat")], ids=[r["id"] for r in ROWS if r.get("sat")])
def test_tables_saturate_as_the_row_says(T, row):
    plan = R.plan_of(row)
    assert plan["rc"] == 0, plan["msg"]
    if row["entry"] == "chain":          # (a single chain: the acceptance thresholds alone)
        t32, t44 = plan["acc_thr"][0], plan["acc_thr44"][0]
        assert (t32[3] == 1 and t44[3] == 1) if row["sat"] == "thr44" else ((t32 == 0).all() and (t44 == 0).all())
        return
    _saturation(row, plan)
    print("%-44s acc_thr[0]=%s acc_thr44[0]=%s swap_thr[0][1:4]=%s swap_inv_log2=%s" % (row["id"], plan["acc_thr"][0].tolist(), plan["acc_thr44"][0].tolist(),
                                                                                 plan["swap_thr"][0][1:4].tolist(), plan["swap_inv_log2"].tolist()))
    if row["scan"] != "wave":
        return
    # the wave kernels' bound on these rows against the brute-force maximum, at 0, 1, 2, every entry and its two neighbours, and 2^32 - 1
    pr, nq = R.block_of(row), plan["nq"]
    for pair in range(row["Nc"] - 1):
        thr = plan["swap_thr"][pair].astype(np.int64)
        xs = np.concatenate([thr[1:] - 1, thr[1:], thr[1:] + 1, np.array([0, 1, 2, 2**32 - 1], np.int64)])
        xs = np.unique(xs[(xs >= 0) & (xs < 2**32)]).astype(np.uint32)
        got = np.zeros(xs.size, np.uint32)
        assert T.qt_wave_swap_bound(C.byref(pr), pair, xs.ctypes.data, xs.size, got.ctypes.data) == nq
        passes = xs[:, None].astype(np.uint64) < plan["swap_thr"][pair][None, 1:]
        brute = np.where(passes.any(axis=1), nq - np.argmax(passes[:, ::-1], axis=1), 0)
        assert np.array_equal(got, brute.astype(np.uint32)), (pair, xs.tolist(), got.tolist(), brute.tolist())


# ---------------------------------------------------------------------------------------------------------------- (c)
RUN = [r for r in ROWS if "refusal" not in r]


@pytest.mark.parametrize("row", RUN, ids=[r["id"] for r in RUN])
def test_the_oracles_run_is_not_vacuous(orc, row):
    init = R.make_init(row)
    ref = R.run_oracle(orc, row, init)
    why = R.vacuous(orc, row, init, ref)
    if "swap_accepts" in ref:
        print("%-44s swaps accepted per pair %s of %d%s" % (row["id"], ref["swap_accepts"].sum(axis=0).tolist(), row["N"] * row["steps"],
                                                          "".join("; %s: %s" % kv for kv in row["weaker"].items())))
    assert why == []
    if row["weaker"].get("swaps") in R.NEAR_BITS:          # the reason the row gives for "every swap accepted" is true of the plan's own rows
        assert (R.plan_of(row)["swap_thr"][:, 1:] > (1 << 32) - (1 << (32 - R.NEAR_BITS[row["weaker"]["swaps"]]))).all()


# ---------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("p", [1e-300, R.MIN_DOUBLE], ids=["1e-300", "min"])
@pytest.mark.parametrize("scan", ["random", "wave"])
def test_the_oracle_is_deterministic_at_the_bottom_of_the_range(orc, p, scan):
    row = dict(R.ROW["C %s toric L5 Nc5 p=%s" % (scan, "1e-300" if p == 1e-300 else "min")])
    assert R.p_of(row) == p
    init = R.make_init(row)
    a, b = (R.run_oracle(orc, row, init) for _ in range(2))
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert np.isin(a["states"], (0, 1, 2, 3)).all() and a["samples"].sum() > 0
