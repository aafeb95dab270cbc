"""The exact class law at the ends of float64's range, without a GPU: the host twins of the three sum-product sweeps and of their _site forms, and the
law functions of qecmc.exact, against the law in exact rational arithmetic (tests/util_rational_law.py).

The sweeps work in ratio form (1, f, f, f) with no rescaling, so a class weight is about count * f^cost and leaves the normal range at low p.  What is
pinned: down a ladder of f that takes every row's total from 1e-250 through the subnormals to 0, the twins return what IEEE arithmetic gives -- right to
1e-12 while normal, within a counted number of subnormal roundings below, exactly 0 at the bottom, never negative, never NaN -- and the law functions
either answer within 1e-12 absolute of the rational law or raise FloatingPointError naming the first offending row; they may not refuse while the
exact total is >= 2^-960.  At the other end weights above 1 take Z to inf, which is refused by name and never normalised to NaN.

ROWS are picked on the reference alone: at each shape one syndrome whose two most likely classes tie in least cost with different counts (found with
tests/util_minplus.py and asserted) -- where a rounded subnormal shows in the law -- and one with a single dominant class.

The sweeps themselves need a device, so on the host the three sweep routes of exact_class_probabilities are reached as the twins' Z through
qecmc.exact.law_from_class_weights, the one normaliser both law functions share; the hist= route runs as it is.  tests/test_gpu_class_law_range.py
runs the public functions on the device."""
from fractions import Fraction

import numpy as np
import pytest

import test_class_sweep_cpu as S
import test_class_sweep_cut_cpu as SC
import test_class_sweep_site_cpu as SS
import test_class_sweep_tiled_cpu as ST
import test_enumerate_cpu as E
from qecmc import exact as ex
from test_corrections_cpu import generators
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_minplus import eliminate_minplus
from util_rational_law import FLOOR, TINY, close_to, law, least_cost_and_count, site_class_weights, uniform_class_weights
from util_sectors import order_for

NAME = S.NAME
# (code, L) -> (draws before, draws, the tied row, the row with one dominant class) of random_errors under default_rng(SEED[code, L])
ROWS = {(ROTATED, 5): (6, 6, 2, 5), (XZZX, 5): (0, 12, 7, 8), (ROTATED, 3): (0, 60, 26, 17), (XZZX, 3): (0, 12, 2, 8), (PLANAR, 3): (0, 12, 5, 11),
        (TORIC, 3): (0, 12, 5, 8)}
# (code, L) -> the twins' plans: cut (lds_width,) with held generators; tiled (hbm_width, tile_width), many segments or forced holds
CUT = {(ROTATED, 5): 5, (XZZX, 5): 6, (ROTATED, 3): 2, (XZZX, 3): 2, (PLANAR, 3): 3, (TORIC, 3): 5}
TILED = {(ROTATED, 5): (5, 4), (XZZX, 5): (0, 4), (ROTATED, 3): (0, 4), (XZZX, 3): (0, 4), (PLANAR, 3): (5, 4), (TORIC, 3): (8, 4)}
SHAPES = sorted(ROWS)
KINDS = ("tied", "single")


@pytest.fixture(scope="module")
def T():
    return SS.load_twin()


def draw(code, L):
    """the draw the rows of one shape are taken from.  Rotated L = 5: default_rng(1), random_errors(ROTATED, 3, 6) first, then the six L = 5 chains"""
    before, n = ROWS[code, L][:2]
    rng = np.random.default_rng(1) if (code, L) == (ROTATED, 5) else np.random.default_rng([83, code, L])
    if before:
        random_errors(code, 3, before, rng)
    return random_errors(code, L, n, rng)


_rows = {}


def rows_of(T, code, L):
    """dict(chains uint8[2, ...]: the tied row and the single one, hist: their histograms from the enumerator's twin, least: [(cost, count)] per class
    of either), computed once and left unchanged"""
    if (code, L) not in _rows:
        chains = np.ascontiguousarray(draw(code, L)[list(ROWS[code, L][2:])])
        hist = E.twin(T, code, L, chains)[0]
        for a in (chains, hist):
            a.setflags(write=False)
        _rows[code, L] = dict(chains=chains, hist=hist, least=[least_cost_and_count(h) for h in hist])
    return _rows[code, L]


def plans_of(T, code, L):
    """[(name, twin call on (chains, w4) -> Z, dict(n_ops, n_gen, held) of the plan)]: the three uniform twins at the plans of CUT and TILED"""
    lw, (hw, tw) = CUT[code, L], TILED[code, L]
    return [("sweep", lambda c, w: S.twin(T, code, L, c, w)[0], S.info(T, code, L)[1]),
            ("cut", lambda c, w: SC.twin(T, code, L, c, w, lw)[0], SC.info(T, code, L, lw)[1]),
            ("tiled", lambda c, w: ST.twin(T, code, L, c, w, hw, tw)[0], ST.info(T, code, L, hw, tw)[1])]


def rounding_count(code, L):
    """How many half-units of 2^-1074 the subnormal roundings of a sweep can add up to in one class weight, for weights <= 1.  A sum of subnormals is
    exact; a multiply whose result is subnormal rounds by at most 2^-1075; weights <= 1 never amplify an earlier error.  Every one of the 2^n_gen
    subsets of the generator table the sweep sums over -- swept and held alike, however the plan splits them -- carries one product through one CLOSE
    per qubit a generator touches, so the count is below n_close * 2^n_gen half-units, plus one for the torus' last division by 4.  In units of
    2^-1074: n_close * 2^(n_gen - 1) + 1.  (Roundings in the normal range are relative and covered by the 1e-12 term beside it.)"""
    gens = generators(code, L)
    return int(gens.any(axis=0).sum()) * (1 << (len(gens) - 1)) + 1


def check_raw(z, want, n_ops, count, where):
    """the raw-Z bounds of one row: z float64[ncls] from a twin against the exact class weights want [Fraction]"""
    assert not np.isnan(z).any() and np.all(z >= 0.0), (where, z)
    for c, (got, w) in enumerate(zip(z.tolist(), want)):
        if w >= FLOOR:
            assert close_to(got, w, 1e-12), (where, c, got, float(w))           # relative 1e-12, the sweep tests' own tolerance
        elif w * 2 ** (n_ops + 1) >= TINY:
            # below 2^-960: rounding_count() units of 2^-1074 for the roundings in the subnormal range, next to the relative term of the bound above
            # for those in the normal range (just below 2^-960 a relative 2^-53 alone is 2^60 units: no count of subnormal roundings covers it, so a
            # purely absolute bound would have to be that much looser everywhere)
            assert abs(Fraction(got) - w) <= Fraction(1e-12) * w + count * TINY, (where, c, got, float(w))
        else:
            assert got == 0.0, (where, c, got)                                   # every rounding on the way doubles a value at most: nothing is left


def check_law(call, want_law, total, where, row=0):
    """one law function at one step: the rational law within 1e-12 absolute, or FloatingPointError naming the row -- and no refusal while the exact
    total is >= 2^-960.  Returns (answered, worst absolute error)"""
    try:
        got = call()
    except FloatingPointError as e:
        assert total < FLOOR, (where, "refused at an exact total of %.3g >= 2^-960" % float(total), str(e))
        assert ("row %d" % row) in str(e), (where, str(e))
        return False, 0.0
    assert got.shape[-1] == len(want_law) and not np.isnan(got).any(), (where, got)
    err = max(abs(Fraction(g) - w) for g, w in zip(got.reshape(-1).tolist(), want_law))
    assert err <= Fraction(1e-12), (where, "law off by %.3g at an exact total of %.3g" % (float(err), float(total)), got)
    return True, float(err)


def ladder(least):
    """the p of every step for one row: f steps down geometrically, four steps per decade of the row's total, from a total of 1e-250 to one decade
    past 2^-1074 -- from the row's own least cost and the number of chains that have it"""
    cost = min(c for c, _ in least)
    count = sum(n for c, n in least if c == cost)
    assert cost >= 2
    out = []
    for k in range(4 * (325 - 250) + 1):
        f = 10.0 ** ((-250.0 - k / 4.0 - np.log10(count)) / cost)
        out.append(3.0 * f / (1.0 + 3.0 * f))
    return out


# ------------------------------------------------------------------------------------------------------ the rows, on the reference alone
@pytest.mark.parametrize("code,L", SHAPES)
def test_the_rows_are_what_they_are_picked_for(T, code, L):
    case = rows_of(T, code, L)
    gens, mult = generators(code, L), 4 if code == TORIC else 1
    for k, chain in enumerate(case["chains"]):
        mp = [eliminate_minplus(gens, r, (0, 1, 1, 1), order_for(code, L)) for r in E.class_chains(code, chain)]
        assert [(c, n // mult) for c, n in mp] == case["least"][k]              # the histogram's least cost and count are the (min, +) elimination's
    tied, single = (sorted(x, key=lambda cn: (cn[0], -cn[1])) for x in case["least"])
    print(NAME[code], L, "tied row", tied[:4], "single row", single[:4])
    assert tied[0][0] == tied[1][0] and tied[0][1] != tied[1][1]                # the two most likely classes tie in least cost with different counts
    assert 2 <= single[0][0] < single[1][0]                                     # one dominant class (a least cost of 1 would take f itself off the doubles)
    if (code, L) == (ROTATED, 5):                                               # four classes at least cost 7 with 2, 2, 8 and 12 shortest chains
        assert case["least"][0] == [(7, 2), (7, 2), (7, 8), (7, 12)]
        f = Fraction(1e-46)
        far = law(uniform_class_weights(case["hist"][0], 1e-46, 1e-46))
        assert max(abs(a - b) for a, b in zip(far, (Fraction(1, 12), Fraction(1, 12), Fraction(1, 3), Fraction(1, 2)))) < 10000 * f


# ------------------------------------------------------------------------------------------------------ the ladder
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("code,L", SHAPES)
def test_down_the_ladder_twins_stay_raw_and_laws_are_right_or_refused(T, code, L, kind):
    case = rows_of(T, code, L)
    k = KINDS.index(kind)
    chain, hist, steps = case["chains"][k:k + 1], case["hist"][k], ladder(case["least"][k])
    plans, count = plans_of(T, code, L), rounding_count(code, L)
    seen, table = set(), {}
    for step, p in enumerate(steps):
        w4 = ex.depolarizing_w4(p)
        want = uniform_class_weights(hist, w4[1], w4[3])                        # the very weights the sweep is given
        total, want_law = sum(want), law(want)
        if step == 0:
            assert Fraction(0.99e-250) < total < Fraction(1.01e-250)
        seen.add("normal" if total >= Fraction(1, 2 ** 1022) else "subnormal" if total >= TINY else "zero")
        for name, run, inf in plans:
            where = (NAME[code], L, kind, name, "f=%.4g" % w4[1])
            z = run(chain, w4)
            check_raw(z[0], want, inf["n_ops"], count, where)
            answered, _ = check_law(lambda: ex.law_from_class_weights(z), want_law, total, where)
            if name == "sweep" and z.sum() > 0:                                 # what a bare z / z.sum() would have returned, for the record
                raw = max(abs(Fraction(g) - w) for g, w in zip((z[0] / z[0].sum()).tolist(), want_law))
                table[step] = (w4[1], float(total), float(raw), answered)
        check_law(lambda: ex.exact_class_probabilities(NAME[code], None, p, hist=hist[None]), want_law, total, (NAME[code], L, kind, "hist", "p=%.4g" % p))
    assert total < TINY / 10 and seen == {"normal", "subnormal", "zero"}        # the three ranges are all crossed
    for step in (s for s in sorted(table) if s % 40 == 0 or (s >= 220 and s % 4 == 0) or s >= 280):
        print("%s L=%d %s: f %.3g, exact total %.3g, a bare z / z.sum() errs by %.3g, %s" % ((NAME[code], L, kind) + table[step][:3] + ("answered" if table[step][3] else "refused",)))
    if kind == "tied":                                                          # these rows are where a rounded subnormal shows: a bare division is wrong there
        assert max(v[2] for v in table.values()) > 1e-3


def test_the_refusal_names_the_first_offending_row(T):
    """rotated L = 5 at f = 1e-46: the single row (least cost 6) totals about 5e-276, the tied row (least cost 7) about 2.4e-321"""
    case = rows_of(T, ROTATED, 5)
    w4 = np.array([1.0, 1e-46, 1e-46, 1e-46])
    chains = case["chains"][[1, 1, 0, 1, 0]]
    z, _ = S.twin(T, ROTATED, 5, chains, w4)
    with pytest.raises(FloatingPointError, match=r"row 2: .*below 2\^-960.*underflow"):
        ex.law_from_class_weights(z)
    good = ex.law_from_class_weights(z[[0, 1, 3]])
    want = law(uniform_class_weights(case["hist"][1], 1e-46, 1e-46))
    assert max(abs(Fraction(g) - w) for g, w in zip(good[2].tolist(), want)) <= Fraction(1e-12)
    # a class that underflows to 0 beside a comfortably normal total stays allowed
    got = ex.law_from_class_weights(np.array([[1e-200, 0.0, 5e-324, 1e-200]]))
    assert got[0, 0] == got[0, 3] == 0.5 and got[0, 1] == 0.0 and 0.0 < got[0, 2] < 2.0 ** -60
    with pytest.raises(FloatingPointError, match="^every class weight of a syndrome underflows to 0 in float64: the law of that row is not representable"):
        ex.law_from_class_weights(np.array([[1.0, 1.0], [0.0, 0.0]]))
    with pytest.raises(FloatingPointError, match="row 1"):
        ex.law_from_class_weights(np.array([[1.0, 1.0], [0.0, 0.0]]))


# ------------------------------------------------------------------------------------------------------ the top of the range
def site_plans(code, L):
    """[(route, widths)] of the three site twins at the plans of CUT and TILED"""
    return [("sweep", ()), ("cut", (CUT[code, L],)), ("tiled", TILED[code, L])]


def test_overflow_is_inf_from_the_twins_and_refused_by_name(T):
    chains = rows_of(T, ROTATED, 3)["chains"]
    big = np.array([1e120, 1.0, 1.0, 1.0])
    for name, run, _ in plans_of(T, ROTATED, 3):
        z = run(chains, big)
        assert np.all(np.isinf(z)) and np.all(z > 0), (name, z)                 # what IEEE gives, on all four classes
        with pytest.raises(FloatingPointError, match="row 0: .*overflow"):
            ex.law_from_class_weights(z)
    # a site table per syndrome whose second row has ratios 1e40 on every qubit
    wq = np.broadcast_to(ex.depolarizing_w4(0.1), (2, 9, 4)).copy()
    wq[1, :, 1:] = 1e40
    for route, widths in site_plans(ROTATED, 3):
        z, _ = SS.twin(T, route, ROTATED, 3, chains, wq, widths)
        assert not np.isnan(z).any() and np.all(np.isfinite(z[0])) and np.isinf(z[1]).any(), (route, z)
        with pytest.raises(FloatingPointError, match="row 1: .*overflow"):
            ex.law_from_class_weights(z)
        assert np.all(np.isfinite(ex.law_from_class_weights(z[:1])))


@pytest.mark.parametrize("code", [XZZX, ROTATED, PLANAR])
def test_weights_above_one_that_stay_finite_are_answered(T, code):
    """ratio 1e6 on three qubits: the law to 1e-12 against the brute force"""
    case = rows_of(T, code, 3)
    gens = generators(code, 3)
    nq = int(np.prod(state_shape(code, 3)))
    wq = np.broadcast_to(ex.depolarizing_w4(0.1), (nq, 4)).copy()
    wq[np.flatnonzero(gens.any(axis=0))[[0, 4, 7]], 1:] = 1e6
    want = site_class_weights(gens, E.class_chains(code, case["chains"][0]), wq)
    for route, widths in site_plans(code, 3):
        z, _ = SS.twin(T, route, code, 3, case["chains"][:1], wq, widths)
        assert all(close_to(g, w, 1e-12) for g, w in zip(z[0].tolist(), want)) and z.max() > 1e6
        check_law(lambda: ex.law_from_class_weights(z), law(want), sum(want), (NAME[code], route))


# ------------------------------------------------------------------------------------------------------ site tables near the bottom
N_TABLES = 16
# code -> [(the table of the tied row, the table of the single row)]: the first pair is one table for both syndromes, the others one per syndrome.
# Picked on the twin's output so that class weights land in the normal range, the subnormals and on 0, and rows total 0, less than 2^-960 and more
BOTTOM = {XZZX: [(10, 10), (11, 12), (6, 8)], ROTATED: [(11, 11), (10, 12), (6, 10)], PLANAR: [(6, 6), (5, 10), (7, 11)]}


def bottom_tables(code):
    """N_TABLES site tables: per-qubit f_q spread log-uniformly over 30 decades, which start at 1e-20 and move down 12 decades from table to table;
    two cells erased (1, 1, 1, 1) and two noiseless (1, 0, 0, 0) in each: float64[N_TABLES, nq, 4]"""
    nq = int(np.prod(state_shape(code, 3)))
    rng = np.random.default_rng([89, code])
    out = np.zeros((N_TABLES, nq, 4))
    for t in range(N_TABLES):
        f = 10.0 ** -(20.0 + 12.0 * t + rng.uniform(0.0, 30.0, size=nq))
        out[t] = np.stack([np.ones(nq), f, f, f], axis=1)
        cells = rng.permutation(np.flatnonzero(generators(code, 3).any(axis=0)))[:4]
        out[t, cells[:2]] = 1.0
        out[t, cells[2:]] = [1.0, 0.0, 0.0, 0.0]
    return out


def bottom_cases(code):
    """[(wq: one table [1, nq, 4] or one per syndrome [2, nq, 4], the pair of table indices)] of BOTTOM"""
    tables = bottom_tables(code)
    return [(tables[[a]] if a == b else tables[[a, b]], (a, b)) for a, b in BOTTOM[code]]


@pytest.mark.parametrize("code", [XZZX, ROTATED, PLANAR])
def test_site_tables_near_the_bottom(T, code):
    """the three site twins under one table for both rows, and under a table per syndrome, against the site brute force"""
    case = rows_of(T, code, 3)
    gens, chains, tables = generators(code, 3), case["chains"], bottom_tables(code)
    reps = [E.class_chains(code, m) for m in chains]
    count, zones, totals = rounding_count(code, 3), set(), set()
    infos = {"sweep": S.info(T, code, 3)[1], "cut": SC.info(T, code, 3, CUT[code, 3])[1], "tiled": ST.info(T, code, 3, *TILED[code, 3])[1]}
    for wq, pick in bottom_cases(code):
        assert len(wq) == (1 if pick[0] == pick[1] else 2)
        want = [site_class_weights(gens, reps[s], tables[pick[s]]) for s in range(2)]
        for w in (x for row in want for x in row):
            zones.add("normal" if w >= FLOOR else "zero" if w * 2 ** 40 < TINY else "low")
        for route, widths in site_plans(code, 3):
            z, _ = SS.twin(T, route, code, 3, chains, wq, widths)
            for s in range(2):
                where = (NAME[code], route, pick, s)
                check_raw(z[s], want[s], infos[route]["n_ops"], count, where)
                if sum(want[s]) > 0:
                    answered, _ = check_law(lambda: ex.law_from_class_weights(z[s:s + 1]), law(want[s]), sum(want[s]), where)
                    totals.add("answered" if answered else "refused")
                else:
                    with pytest.raises(FloatingPointError, match="^every class weight of a syndrome underflows to 0.*row 0"):
                        ex.law_from_class_weights(z[s:s + 1])
                    totals.add("zero")
    print(NAME[code], "class weights met:", sorted(zones), "rows:", sorted(totals))
    assert zones == {"normal", "low", "zero"} and "answered" in totals and len(totals) >= 2
