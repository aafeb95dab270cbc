"""The exact chain sampler and the exact marginals at the ends of float64's range, without a GPU: the host twins (qt_class_sample, qt_class_marginals),
the record of one job (qt_class_sample_record) and the Python layer of qecmc.exact, against the law of a chain and the marginals of a class in exact
rational arithmetic (tests/util_rational_sample.py).  Both families run on the raw, unrescaled sum-product sweep, and the rule they are held to is
the class law's: RIGHT, OR REFUSED BY NAME.

SUPPORT, at every range: whenever a sampler call is answered, every drawn chain has exact weight > 0 and its class an exact Z_c > 0.  The one-chain
tables give every qubit one Pauli of positive weight, so one chain of the whole syndrome has weight > 0, and scale it from 1e-90 to the last positive
double; the mixed table makes the record's pairs subnormal under a class weight above the floor, so that an ANSWERED call walks forced branches
through s = 2^-1074, where u * s rounds back up to s.

THE LAW, without draws.  From the record of a job the probability THE RULE of csrc/class_sample.hpp gives every chain of the coset is a product of
per-FORGET probabilities #{m in [0, 2^53): fl(m 2^-53 s) < on || on == s} / 2^53 -- counted by bisection on m with float64 multiplies, the product
being monotone in m --, times the class pick's and the held pick's, counted the same way.  That the twin's walk IS this rule is pinned by replaying
its draws (test_the_twins_draws_are_the_rule_replayed).  The rule's law is within 1e-12 total variation of the rational law wherever a call is
answered.  Why 1e-12 is reachable at L = 3 (n_forget <= 8 FORGETs of a job, n_ops < 64, width <= 6, weights <= 1, Z_c >= 2^-961):
  * one rounding per add and per multiply: a pair (on, s) of normal doubles carries a relative error below 2 n_ops 2^-53 each, so on / s is off by
    less than 4 n_ops 2^-53 relative, and a product of n_forget such ratios by 4 n_ops n_forget 2^-53 < 2^-42 relative: 2.3e-13 of total variation at most;
  * the 2^-53 grain of u and the rounding of u * s: a branch's count is off from 2^53 on / s by at most 2, an absolute 2^-52 per FORGET on the mass
    that reaches it, n_forget 2^-52 < 2^-49 summed along a path and over the tree;
  * paths through subnormal states, where the ratios mean nothing: a state below 2^-1022 carries at most 2^-1022 / 2^-961 = 2^-61 of the class, and
    there are fewer than n_forget 2^width of them: 2^(-61 + 3 + 6) = 2^-52 at most (the crude 2^(-62 + n_gen + width) of DESIGN.md 4.1s holds as well);
  * the picks: one count each, 2^-52, and the running sums' roundings, 16 2^-53 relative.
The sum is below 3e-13.  The total variation is evaluated in float64 from correctly rounded quotients of integers: 2^-52 per chain's mass, 2^-51 in all.

RIGHT OR REFUSED.  A sampler refusal names the row, the class in every-class mode, and the end of the range it met, and is never raised while the
exact Z_c (every-class mode) or the exact row total (posterior mode) is >= 2^-960; the four marginal functions answer within 1e-12 absolute of the
rational values (exact_error_counts: 1e-12 times the number of qubits) or raise FloatingPointError naming the row and the class, never at or above
2^-960; normalize=False stays raw.  The Python functions are reached on the host as tests/test_class_marginal_cpu.py reaches them: the twin's output
in place of the device's, through the same normalising code.

Worst figures printed by these tests: see DESIGN.md 4.1s and 4.1t, "Range"."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import sample_range_cases as RC
import test_class_law_range_cpu as R
import test_class_marginal_cpu as MA
import test_class_sample_cpu as SA
import test_enumerate_cpu as E
import util_class_sample as U
import util_rational_sample as Q
from qecmc import exact as ex
from test_corrections_cpu import generators
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, state_shape
from util_rational_law import FLOOR, TINY, uniform_class_weights

NAME = R.NAME
SHAPES = [(ROTATED, 3), (XZZX, 3)]
KINDS = R.KINDS
TWO53 = 1 << 53
SEED = RC.SEED
_f64p, _u32p, _u8p = SA._f64p, SA._u32p, SA._u8p


@pytest.fixture(scope="module")
def T():
    lib = MA.load_twin()
    lib.qt_class_sample_record.restype = C.c_int
    lib.qt_class_sample_record.argtypes = [C.c_int, C.c_int, _u8p, _f64p, _f64p, C.c_int, C.c_int, C.c_uint32, _f64p, C.c_uint64, _f64p, _f64p, _u32p, _u32p, C.c_int]
    lib.qt_class_sample_floor.restype = C.c_double
    return lib


# ------------------------------------------------------------------------------------------------------ the record of one job, and the rule on it
_plans = {}


def plan_of(T, code, L, lds_width):
    """dict(n_forget, W, width, held, forget_words uint32[n_forget, W]) of the sampler's plan"""
    if (code, L, lds_width) not in _plans:
        pn = SA.plan_numbers(T, code, L, lds_width)
        words = np.zeros((pn["n_forget"], pn["W"]), np.uint32)
        assert T.qt_class_sample_plan(code, L, lds_width, None, words.ctypes.data_as(_u32p), words.size, None) == pn["n_forget"]
        _plans[code, L, lds_width] = dict(pn, forget_words=[[int(x) for x in row] for row in words])
    return _plans[code, L, lds_width]


def record_of(T, code, L, chain, cls, h=0, w=None, wq=None, lds_width=0):
    """one job of the twin: dict(pairs float64[n_forget, 2^(width-1), 2] as (on, s), partials float64[2^held] of the class, z float64[ncls], rep [int] * W:
    the chain the walk starts from, ops [int]: word 0 of every op)"""
    pl = plan_of(T, code, L, lds_width)
    nq, ncls = RC.nq_of(code, L), 16 if code == TORIC else 4
    pairs = np.full((pl["n_forget"], 1 << (pl["width"] - 1), 2), -1.0)
    partials, z, rep, ops = np.full(1 << pl["held"], -1.0), np.full(ncls, -1.0), np.zeros(pl["W"], np.uint32), np.zeros(4096, np.uint32)
    flat = np.ascontiguousarray(chain, dtype=np.uint8).reshape(nq)
    wp = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    tab = None if wq is None else np.ascontiguousarray(wq, dtype=np.float64).reshape(nq, 4)
    n = T.qt_class_sample_record(code, L, flat.ctypes.data_as(_u8p), None if wp is None else wp.ctypes.data_as(_f64p), None if tab is None else tab.ctypes.data_as(_f64p),
                                 lds_width, cls, h, pairs.ctypes.data_as(_f64p), pairs.size // 2, partials.ctypes.data_as(_f64p), z.ctypes.data_as(_f64p),
                                 rep.ctypes.data_as(_u32p), ops.ctypes.data_as(_u32p), ops.size)
    assert n > 0
    return dict(pairs=pairs, partials=partials, z=z, rep=[int(x) for x in rep], ops=[int(x) for x in ops[:n]], plan=pl, nq=nq)


def below_count(s, on):
    """#{m in [0, 2^53): fl(m 2^-53 * s) < on} for doubles s >= on >= 0: the product is monotone in m, so the count is the least m that fails,
    found by bisection with float64 multiplies (m 2^-53 is exact); a guess from the quotient narrows the bracket first"""
    if not on > 0.0:
        return 0
    passes = lambda m: (m * 2.0 ** -53) * s < on
    if passes(TWO53 - 1):
        return TWO53
    lo, hi = 0, TWO53 - 1                                                       # passes(lo), not passes(hi)
    guess = on / s * 9007199254740992.0
    if guess == guess and guess < 9007199254740992.0:
        a, b = max(int(guess) - 4, 0), min(int(guess) + 4, TWO53 - 1)
        if passes(a) and not passes(b):
            lo, hi = a, b
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if passes(mid) else (lo, mid)
    return hi


def take_count(on, s):
    """of 2^53 uniforms, how many take the branch: u * s < on || on == s"""
    return TWO53 if on == s else below_count(s, on)


def pick_counts(v):
    """of 2^53 uniforms, how many pick each index of v: the lowest i with u * last < run_i || run_i == last, sequential float64 adds in ascending order"""
    v = [float(x) for x in v]
    last = v[0]
    for x in v[1:]:
        last = last + x
    out, run, before = [], v[0], 0
    for i in range(len(v)):
        upto = TWO53 if (run == last or i == len(v) - 1) else below_count(last, run)
        out.append(upto - before)
        before = upto
        if i + 1 < len(v):
            run = run + v[i + 1]
    return out


def remove_bit(f, slot):
    return ((f >> (slot + 1)) << slot) | (f & ((1 << slot) - 1))


def chain_bytes(words, nq):
    return bytes((words[q >> 4] >> (2 * (q & 15))) & 3 for q in range(nq))


def walk(rec, take):
    """step 4 of THE RULE on one record.  take(fi, on, s, states) decides: the walk is followed over every branch (take None: -> {chain bytes: the
    numerator of its probability over 2^(53 n_forget)}) or along one path (take a function (fi, on, s) -> bool: -> the chain's bytes)"""
    pl, pairs = rec["plan"], rec["pairs"]
    states = [(0, tuple(rec["rep"]), 1)]
    fi = pl["n_forget"]
    for w0 in reversed(rec["ops"]):
        kind, slot = w0 & 15, (w0 >> 4) & 15
        bit = 1 << slot
        if kind == KIND["intro"]:
            states = [(f & ~bit, c, n) for f, c, n in states]
        elif kind == KIND["forget"]:
            fi -= 1
            words = pl["forget_words"][fi]
            nxt = []
            for f, c, n in states:
                on, s = (float(x) for x in pairs[fi, remove_bit(f, slot)])
                taken = tuple(a ^ b for a, b in zip(c, words))
                if take is not None:
                    nxt.append((f | bit, taken, n) if take(fi, on, s) else (f, c, n))
                    continue
                k = take_count(on, s)
                if k:
                    nxt.append((f | bit, taken, n * k))
                if TWO53 - k:
                    nxt.append((f, c, n * (TWO53 - k)))
            states = nxt
    assert fi == 0 and all(f == 0 for f, _, _ in states)
    if take is not None:
        return chain_bytes(states[0][1], rec["nq"])
    return {chain_bytes(c, rec["nq"]): n for _, c, n in states}


KIND = {"intro": 0, "close": 1, "forget": 2}                                    # the op kinds of csrc/class_sweep_ops.hpp, bits 0-3 of word 0; the slot is bits 4-7


def rule_law(T, code, L, chain, cls, w=None, wq=None, lds_width=0):
    """({chain bytes: probability numerator}, the denominator's exponent, z float64[ncls]) the rule gives class cls: the held pick times the walk"""
    rec = record_of(T, code, L, chain, cls, 0, w=w, wq=wq, lds_width=lds_width)
    held, nf = rec["plan"]["held"], rec["plan"]["n_forget"]
    if held == 0:
        return walk(rec, None), 53 * nf, rec["z"]
    out = {}
    for h, k in enumerate(pick_counts(rec["partials"])):
        if k:
            for c, n in walk(record_of(T, code, L, chain, cls, h, w=w, wq=wq, lds_width=lds_width), None).items():
                assert c not in out
                out[c] = n * k
    return out, 53 * (nf + 1), rec["z"]


def total_variation(rule, bits, law):
    """half the sum over the coset of |rule / 2^bits - num / total|, in float64 from correctly rounded quotients; a chain outside the coset fails"""
    index = law.index()
    assert set(rule) <= set(index), "the rule reaches a chain outside the class"
    assert sum(rule.values()) == 1 << bits                                      # the rule's law is a law
    tv = 0.0
    for c, i in index.items():
        tv += abs(rule.get(c, 0) / (1 << bits) - law.num[i] / law.total)
    return 0.5 * tv


# ------------------------------------------------------------------------------------------------------ the yardstick, pinned in the normal range
_cosets = {}


def cosets_of(T, code, L, k):
    """the cosets of the classes of row k (0 tied, 1 single) of the shape: [uint8[256, nq]] * ncls, computed once"""
    if (code, L, k) not in _cosets:
        reps = E.class_chains(code, R.rows_of(T, code, L)["chains"][k])
        _cosets[code, L, k] = [Q.coset_of(generators(code, L), r) for r in reps]
    return _cosets[code, L, k]


def laws_of(T, code, L, k, w):
    gens = generators(code, L)
    wt = Q.Weights(gens, w)
    return [Q.CosetLaw(gens, None, wt, coset=c) for c in cosets_of(T, code, L, k)]


_uniform = {}


def uniform_laws_of(T, code, L, k, w4):
    """laws_of under (1, f, f, f), through the counts of util_rational_sample.UniformCoset (pinned against laws_of in the yardstick's test)"""
    assert w4[0] == 1.0 and w4[1] == w4[2] == w4[3]
    if (code, L, k) not in _uniform:
        _uniform[code, L, k] = [Q.UniformCoset(generators(code, L), c) for c in cosets_of(T, code, L, k)]
    return [u.at(w4[1]) for u in _uniform[code, L, k]]


@pytest.mark.parametrize("code,L", SHAPES)
def test_the_rational_yardstick_in_the_normal_range(T, code, L):
    """p = 0.1: against util_class_sample.class_law and the brute force of test_class_marginal_cpu.py, which share no code with it"""
    w = ex.depolarizing_w4(0.1)
    chain = R.rows_of(T, code, L)["chains"][0]
    laws = laws_of(T, code, L, 0, w)
    brute, zs = MA.brute_marginals(code, L, chain, w)
    cells = Q.touched_cells(generators(code, L))
    hist = uniform_class_weights(R.rows_of(T, code, L)["hist"][0], w[1], w[3])
    for c, (chains, prob, zc) in enumerate(U.class_law(code, L, chain, w)):
        assert np.array_equal(chains, laws[c].chains) and len(chains) == 256
        assert laws[c].z == hist[c]                                             # the histogram's class weight, exactly
        assert abs(float(laws[c].z) - zc) <= 1e-14 * zc
        assert max(abs(float(a) - b) for a, b in zip(laws[c].law(), prob)) <= 1e-15
        assert sum(laws[c].law()) == 1
        m = laws[c].marginals()
        for q in cells:
            assert sum(m[q]) == 1
            assert max(abs(float(m[q][P]) * zc - brute[c, q, P]) for P in range(4)) <= 1e-14 * zc
    post = Q.posterior_marginals(laws)
    want = brute.sum(axis=0) / zs.sum()
    assert max(abs(float(post[q][P]) - want[q, P]) for q in cells for P in range(4)) <= 1e-14
    tab = np.broadcast_to(w, (RC.nq_of(code, L), 4))                            # the site form of the same weights is the same law
    assert [x.num for x in laws_of(T, code, L, 0, tab)] == [x.num for x in laws]
    fast = uniform_laws_of(T, code, L, 0, w)                                    # ... and the counted form the ladders use
    for a, b in zip(fast, laws):
        assert a.z == b.z and a.law() == b.law() and a.marginals() == b.marginals()


def test_the_floor_is_the_law_functions_floor(T):
    assert T.qt_class_sample_floor() == ex.LAW_FLOOR == 2.0 ** -961 and Fraction(ex.LAW_FLOOR) * 2 == FLOOR


def test_counts_of_the_rule():
    assert take_count(5e-324, 5e-324) == TWO53 and below_count(5e-324, 5e-324) == (1 << 52) + 1   # 0.75 * 5e-324 == 5e-324: the first compare alone declines every u > 1/2 (at 1/2 the tie rounds to 0)
    assert take_count(0.0, 1.0) == 0 and take_count(0.25, 1.0) == 1 << 51 and take_count(1.0, 1.0) == TWO53
    assert below_count(1.0, 1.0) == TWO53                                       # in the normal range on == s is implied: u * s < s for every u
    assert below_count(3.0, 1.0) == -(-TWO53 // 3)
    assert pick_counts([1.0, 0.0, 1.0, 0.0]) == [1 << 52, 0, 1 << 52, 0]
    assert pick_counts([1e-323, 2e-323, 0.0, 0.0])[2:] == [0, 0] and pick_counts([0.0, 5e-324, 0.0]) == [0, TWO53, 0]
    assert sum(pick_counts([0.3, 0.2, 0.1, 0.4])) == TWO53


# ------------------------------------------------------------------------------------------------------ the twin's walk is the rule
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 3, 0), (XZZX, 3, 0), (ROTATED, 3, 2)])
def test_the_twins_draws_are_the_rule_replayed(T, code, L, lds_width):
    """every draw of the twin, replayed in Python on the record with the documented uniforms, at a normal step and at the last answered one"""
    case = R.rows_of(T, code, L)
    ncls, K = 4, 16
    held = plan_of(T, code, L, lds_width)["held"]
    assert (held > 0) == (lds_width != 0)
    steps = R.ladder([max(case["least"][0])])
    for step in (0, 150):
        w4 = ex.depolarizing_w4(steps[step])
        out, _, z = SA.twin(T, code, L, case["chains"][:1], w=w4, K=K, seed=SEED, first=5, lds_width=lds_width)
        post, cls, _ = SA.twin(T, code, L, case["chains"][:1], w=w4, K=K, seed=SEED, first=5, mode=1, lds_width=lds_width)
        for k in range(K):
            counts = pick_counts(z[0])
            m = int(U.u53(SEED, 5, ncls, k, 0, 0) * TWO53)
            assert cls[0, k] == next(c for c in range(ncls) if m < sum(counts[:c + 1]))
            assert np.array_equal(post[0, k], out[0, cls[0, k], k])
        for c in range(ncls):
            recs = {}
            for k in range(K):
                h = 0
                if held:
                    counts = pick_counts(record_of(T, code, L, case["chains"][0], c, 0, w=w4, lds_width=lds_width)["partials"])
                    m = int(U.u53(SEED, 5, c, k, 0, 0) * TWO53)
                    h = next(i for i in range(len(counts)) if m < sum(counts[:i + 1]))
                if h not in recs:
                    recs[h] = record_of(T, code, L, case["chains"][0], c, h, w=w4, lds_width=lds_width)
                got = walk(recs[h], lambda fi, on, s: U.u53(SEED, 5, c, k, 1 + (fi >> 1), fi & 1) * s < on or on == s)
                assert got == out[0, c, k].tobytes(), (step, c, k)


@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 3, 0), (XZZX, 3, 0), (ROTATED, 3, 2)])
def test_the_rules_law_at_p_0_1(T, code, L, lds_width):
    """far from either end, where no branch is forced and the walk's tree is full: the same 1e-12, in both modes, under biased weights as well"""
    chain = R.rows_of(T, code, L)["chains"][0]
    for w in (ex.depolarizing_w4(0.1), SA.BIASED, SA.FLAT):
        laws = laws_of(T, code, L, 0, w)
        rules = [rule_law(T, code, L, chain, c, w=w, lds_width=lds_width) for c in range(4)]
        assert all(len(rule) == 256 for rule, _, _ in rules)
        worst = max(total_variation(rule, bits, laws[c]) for c, (rule, bits, _) in enumerate(rules))
        picks, total = pick_counts(rules[0][2]), sum(x.total for x in laws)
        tv = 0.5 * sum(abs(picks[c] * rule.get(b, 0) / (1 << (bits + 53)) - laws[c].num[i] / total)
                       for c, (rule, bits, _) in enumerate(rules) for b, i in laws[c].index().items())
        print("%s L=%d lds_width=%d w=%s: total variation %.3g (every class, worst), %.3g (posterior)" % (NAME[code], L, lds_width, np.round(w, 3).tolist(), worst, tv))
        assert worst <= 1e-12 and tv <= 1e-12


# ------------------------------------------------------------------------------------------------------ support: the one-chain tables
def far_chain(gens, chain):
    """the input chain times every other generator (all of them multiply to the identity on the torus): the same syndrome and class, and about half
    of the walk's FORGETs are forced takes, the others forced declines"""
    out = np.asarray(chain, dtype=np.uint8).reshape(-1).copy()
    for g in gens[::2]:
        out ^= g
    assert (out != np.asarray(chain).reshape(-1)).any()
    return out


def one_chain_scales():
    """2^-e: from 1e-90 down to the last positive double, every eighth power of two, and every one below 2^-1060"""
    return [2.0 ** -e for e in list(range(299, 1060, 8)) + list(range(1060, 1075))]


def check_one_chain(rc, msg, samples, cls, want_chain, want_cls, total, where):
    """an answered call returns the chain K times, in its class; a refusal names row 0 and is not raised at or above 2^-960"""
    if rc != 0:
        assert Fraction(total) < FLOOR and "row 0" in msg and "below 2^-960" in msg, (where, msg)
        return False
    wrong = int((samples.reshape(-1, samples.shape[-1]) != want_chain).any(axis=1).sum())
    assert wrong == 0 and (cls == want_cls).all(), (where, "%d of %d samples are not the one chain of weight > 0; classes drawn %s" %
                                                    (wrong, samples.reshape(-1, samples.shape[-1]).shape[0], np.unique(cls).tolist()))
    return True


@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 3, 0), (XZZX, 3, 0), (TORIC, 3, 6)])
def test_one_chain_site_tables_down_to_the_last_positive_double(T, code, L, lds_width):
    K = 4096 if lds_width == 0 else 64
    chain = R.rows_of(T, code, L)["chains"][1]
    gens = generators(code, L)
    flat = far_chain(gens, chain)
    seen = set()
    for scale in one_chain_scales():
        tab = Q.one_chain_table(gens, flat, scale)
        wt = Q.Weights(gens, tab)
        assert wt.weight(flat.tolist()) == Fraction(scale)
        rc, msg, post, cls, z = SA.twin_rc(T, code, L, chain[None], wq=tab, K=K, seed=SEED, mode=1, lds_width=lds_width)
        live = np.flatnonzero(z[0] > 0) if rc == 0 else None
        if rc == 0:
            assert len(live) == 1 and z[0, live[0]] == scale                    # powers of two: the sweep is exact
        seen.add(check_one_chain(rc, msg, post, cls, flat, None if live is None else live[0], scale, (NAME[code], "mode 1", scale)))
        # every-class mode: the other classes are empty, and the first of them is refused by name, as before
        rc, msg, *_ = SA.twin_rc(T, code, L, chain[None], wq=tab, K=4, seed=SEED, mode=0, lds_width=lds_width)
        assert rc == -1 and "row 0, class" in msg and ("is 0 --" in msg or "below 2^-960" in msg), msg
    assert seen == {True, False}


def test_one_chain_four_weights(T):
    """(x, 0, 0, 0) under the trivial syndrome: the empty chain alone, Z = x^9"""
    zero = np.zeros((1, 3, 3), np.uint8)
    seen = set()
    for e in list(range(33, 119, 4)) + [119]:
        x = 2.0 ** -e
        rc, msg, post, cls, z = SA.twin_rc(T, ROTATED, 3, zero, w=[x, 0.0, 0.0, 0.0], K=4096, seed=SEED, mode=1)
        if rc == 0:
            assert z[0].tolist() == [2.0 ** (-9 * e), 0.0, 0.0, 0.0]
        seen.add(check_one_chain(rc, msg, post, cls, zero.reshape(-1), 0, Fraction(1, 2 ** (9 * e)), ("four weights", e)))
    assert seen == {True, False}


def mixed_one_chain_table(T, code, L, lds_width):
    """(the input chain uint8[...], the one chain of weight > 0 uint8[nq], the table float64[nq, 4]): the first two CLOSEs of the plan carry 2^-537
    each, the last 2^124, those between them 1 -- the weight of the chain is 2^-950 exactly"""
    gens = generators(code, L)
    start = R.rows_of(T, code, L)["chains"][1]
    chain = far_chain(gens, start)
    order = [int(q) for q in MA.plan_numbers(T, code, L, lds_width)["close_qubit"]]
    tab = np.ones((len(chain), 4))
    for i, q in enumerate(order):
        tab[q] = 0.0
        tab[q, chain[q]] = 2.0 ** -537 if i < 2 else 2.0 ** 124 if i == len(order) - 1 else 1.0
    assert Q.Weights(gens, tab).weight(chain.tolist()) == Fraction(1, 2 ** 950)
    return start, chain, tab


@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 3, 0), (XZZX, 3, 0), (TORIC, 3, 6)])
def test_forced_branches_through_subnormal_pairs_in_an_answered_call(T, code, L, lds_width):
    """A one-chain table whose first two closed qubits bring the state to 2^-1074 and whose last one lifts the class weight back to 2^-950: the call
    is answered, and every FORGET before the lift is a forced branch at the last positive double, which u * s < on alone declines for every u > 1/2.
    (Support is asked of every answered call; the issue's bounds on the LAW are for weights <= 1 and are not asked here -- one chain has no law to miss)"""
    K = 4096 if lds_width == 0 else 64
    start, chain, tab = mixed_one_chain_table(T, code, L, lds_width)
    rc, msg, post, cls, z = SA.twin_rc(T, code, L, start[None], wq=tab, K=K, seed=SEED, mode=1, lds_width=lds_width)
    assert rc == 0, msg
    live = np.flatnonzero(z[0] > 0)
    assert len(live) == 1 and z[0, live[0]] == 2.0 ** -950
    check_one_chain(rc, msg, post, cls, chain, live[0], Fraction(1, 2 ** 950), (NAME[code], "mixed"))
    if lds_width == 0:                                                          # the premise: the record does hold forced pairs at the last positive double
        pairs = record_of(T, code, L, start, int(live[0]), wq=tab)["pairs"]
        assert ((pairs[..., 1] == 5e-324) & (pairs[..., 0] == 5e-324)).any()


# ------------------------------------------------------------------------------------------------------ the sampler down the ladder
def class_ladder(case, k):
    """the ladder of the costliest class of row k: every class stays positive until that one reaches the floor"""
    return R.ladder([max(case["least"][k])])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 3, 0), (XZZX, 3, 0), (ROTATED, 3, 2), (PLANAR, 3, 0)])
def test_down_the_ladder_every_class_is_drawn_by_its_law_or_refused_by_name(T, code, L, lds_width, kind):
    """every-class mode.  lds_width = 2 holds generators: the law then runs over the held pick as well (every fourth answered step).  Planar L = 3
    has 4 096 chains per class and 12 FORGETs (the derivation's 3e-13 grows to 4e-13): its law is computed at every fourth step, the outcome of
    every step is checked as elsewhere"""
    case, k = R.rows_of(T, code, L), KINDS.index(kind)
    chain, hist = case["chains"][k:k + 1], case["hist"][k]
    seen, outcomes, worst = set(), set(), 0.0
    for step, p in enumerate(class_ladder(case, k)):
        w4 = ex.depolarizing_w4(p)
        site = step % 4 == 1                                                    # every fourth step through the site form of the same weights
        kw = dict(wq=np.broadcast_to(w4, (RC.nq_of(code, L), 4))) if site else dict(w=w4)
        want = uniform_class_weights(hist, w4[1], w4[3])
        seen |= {"normal" if x >= Fraction(1, 2 ** 1022) else "subnormal" if x >= TINY else "zero" for x in want}
        rc, msg, out, _, z = SA.twin_rc(T, code, L, chain, K=8, seed=SEED, lds_width=lds_width, **kw)
        where = (NAME[code], L, lds_width, kind, step)
        if rc != 0:
            outcomes.add("refused")
            assert min(want) < FLOOR, (where, "refused while every exact class weight is >= 2^-960", msg)
            c = int(msg.split("row 0, class ")[1].split(":")[0])                # the refusal names the row, the class and the end of the range
            assert want[c] < FLOOR and all(x >= FLOOR / 2 for x in want[:c]) and ("below 2^-960" in msg or "is 0 --" in msg), (where, msg)
            assert msg.startswith("qecmc_class_sample_site: " if site else "qecmc_class_sample: ")
            continue
        outcomes.add("answered")
        if (lds_width and step % 4) or (code == PLANAR and step % 4):
            continue
        laws = uniform_laws_of(T, code, L, k, w4)
        for c in range(4):
            assert laws[c].z == want[c]
            rule, bits, zr = rule_law(T, code, L, chain[0], c, lds_width=lds_width, **kw)
            assert zr.tobytes() == z[0].tobytes()
            tv = total_variation(rule, bits, laws[c])
            worst = max(worst, tv)
            assert tv <= 1e-12, (where, c, tv)
            index = laws[c].index()
            assert all(laws[c].num[index[s.tobytes()]] > 0 for s in out[0, c])  # support: every drawn chain lies in its class with weight > 0
    print("%s L=%d lds_width=%d %s, every-class mode: worst total variation of the rule's law %.3g" % (NAME[code], L, lds_width, kind, worst))
    assert seen == {"normal", "subnormal", "zero"} and outcomes == {"answered", "refused"}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("code,L", SHAPES)
def test_down_the_ladder_the_posterior_is_drawn_by_its_law_or_refused_by_name(T, code, L, kind):
    """posterior mode on the row's own ladder: the class pick times the walk, over the 1 024 chains of the syndrome"""
    case, k = R.rows_of(T, code, L), KINDS.index(kind)
    chain, hist = case["chains"][k:k + 1], case["hist"][k]
    seen, outcomes, worst = set(), set(), 0.0
    for step, p in enumerate(R.ladder(case["least"][k])):
        w4 = ex.depolarizing_w4(p)
        site = step % 4 == 1
        kw = dict(wq=np.broadcast_to(w4, (RC.nq_of(code, L), 4))) if site else dict(w=w4)
        want = uniform_class_weights(hist, w4[1], w4[3])
        total = sum(want)
        seen.add("normal" if total >= Fraction(1, 2 ** 1022) else "subnormal" if total >= TINY else "zero")
        rc, msg, post, cls, z = SA.twin_rc(T, code, L, chain, K=64, seed=SEED, mode=1, **kw)
        where = (NAME[code], L, kind, step)
        if rc != 0:
            outcomes.add("refused")
            assert total < FLOOR, (where, "refused at an exact total of %.3g >= 2^-960" % float(total), msg)
            assert "row 0: the class weights total" in msg and ("below 2^-960" in msg or "total 0 --" in msg), (where, msg)
            continue
        outcomes.add("answered")
        laws = uniform_laws_of(T, code, L, k, w4)
        picks, tv = pick_counts(z[0]), 0.0
        for c in range(4):
            if picks[c] == 0:
                tv += 0.5 * (laws[c].total / sum(x.total for x in laws))    # a class the pick never reaches: its whole mass is missed
                continue
            rule, bits, _ = rule_law(T, code, L, chain[0], c, **kw)
            index = laws[c].index()
            assert set(rule) <= set(index) and sum(rule.values()) == 1 << bits
            all_total = sum(x.total for x in laws)
            tv += 0.5 * sum(abs(picks[c] * rule.get(b, 0) / (1 << (bits + 53)) - laws[c].num[i] / all_total) for b, i in index.items())
            drawn = post[0][cls[0] == c]
            assert all(laws[c].num[index[s.tobytes()]] > 0 for s in drawn) and (laws[c].total > 0 or not len(drawn))
        worst = max(worst, tv)
        assert tv <= 1e-12, (where, tv)
    print("%s L=%d %s, posterior mode: worst total variation of the rule's law %.3g" % (NAME[code], L, kind, worst))
    assert seen == {"normal", "subnormal", "zero"} and outcomes == {"answered", "refused"}


# ------------------------------------------------------------------------------------------------------ the marginals down the ladder
def through_the_twin(T, L):
    """qecmc.exact._marginals on the twin's numbers: the Python layer above it is the code the device's numbers pass through"""
    def run(code_, chains, w, site_weights, size, lds_width):
        code_ = ex._CODES.get(code_, code_)
        wq = None if site_weights is None else np.asarray(site_weights, dtype=np.float64).reshape((-1,) + (RC.nq_of(code_, L), 4))
        out, z, cls = MA.twin(T, code_, L, chains, w=w, wq=wq, lds_width=lds_width)
        return dict(weights=out.reshape(out.shape[:2] + state_shape(code_, L) + (4,)), z=z, cls=cls, width=0, held=0)
    return run


def answered_or_refused(call, may_refuse, names, where):
    """(True, the answer) or (False, None): a FloatingPointError must name `names` and must not be raised unless may_refuse"""
    try:
        return True, call()
    except FloatingPointError as e:
        assert may_refuse, (where, "refused at or above 2^-960", str(e))
        assert names in str(e) and ("below 2^-960" in str(e) or " 0 --" in str(e)), (where, str(e))
        return False, None


def worst_error(got, want):
    """max |got[q][P] - want[q][P]| as a Fraction, got a float array [nq, 4], want [nq][4] Fractions"""
    return max(abs(Fraction(float(g)) - w) for row, wrow in zip(np.asarray(got).reshape(-1, 4).tolist(), want) for g, w in zip(row, wrow))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("code,L,lds_width", [(ROTATED, 3, 0), (XZZX, 3, 0), (ROTATED, 3, 2)])
def test_down_the_ladder_the_marginals_are_right_or_refused_by_name(T, code, L, lds_width, kind, monkeypatch):
    """The raw weights obey the class sweep's bounds (check_raw of tests/test_class_law_range_cpu.py: the rounding count three times the sweep's -- a
    forward product, a backward product and their combination each round once per CLOSE of a subset, none amplified by weights <= 1 -- and exact zeros
    twice as many ops down), and the four functions answer to 1e-12 or refuse by name.  Two ladders per row: the costliest class's for the per-class
    functions, every second step of the row's own for the posterior; the site form at every fourth step"""
    monkeypatch.setattr(ex, "_marginals", through_the_twin(T, L))
    case, k = R.rows_of(T, code, L), KINDS.index(kind)
    chain, hist = case["chains"][k:k + 1], case["hist"][k]
    cells = [int(q) for q in Q.touched_cells(generators(code, L))]
    nq, n_ops, count = RC.nq_of(code, L), MA.plan_numbers(T, code, L, lds_width)["n_ops"], 3 * R.rounding_count(code, L)
    tol, seen, outcomes, worst = Fraction(1e-12), set(), {}, {}
    ladders = [("class", p) for p in class_ladder(case, k)] + [("row", p) for p in R.ladder(case["least"][k])[::2]]
    if lds_width:
        ladders = ladders[::3]                                                  # held generators: the same bounds on a third of the steps
    for step, (which, p) in enumerate(ladders):
        w4 = ex.depolarizing_w4(p)
        site = step % 4 == 1
        table = np.broadcast_to(w4, state_shape(code, L) + (4,))
        want_z = uniform_class_weights(hist, w4[1], w4[3])
        total = sum(want_z)
        laws = uniform_laws_of(T, code, L, k, w4)
        nums = [x.marginal_numerators() for x in laws]
        where = (NAME[code], L, lds_width, kind, which, step)
        # raw
        raw = ex.class_marginals_site(NAME[code], chain, table, lds_width=lds_width, normalize=False) if site else \
            ex.class_marginals(NAME[code], chain, w4=w4, lds_width=lds_width, normalize=False)
        wts, z = raw["weights"].reshape(4, nq, 4), raw["z"][0]
        assert "marginals" not in raw and not np.isnan(wts).any() and (wts >= 0.0).all()
        R.check_raw(z, want_z, n_ops, R.rounding_count(code, L), where)
        seen |= RC.ranges_of(z)
        for q in cells:
            for P in range(4):
                R.check_raw(wts[:, q, P], [Fraction(nums[c][q][P], 1 << laws[c].depth) for c in range(4)], 2 * n_ops, count, where + (q, P))
        if total < TINY / 2 ** 40:
            assert not wts[:, cells].any() and not z.any()                      # exactly 0 at the bottom
        if which == "class":
            ok = min(want_z) >= FLOOR
            low = next((c for c in range(4) if want_z[c] < FLOOR), 0)
            first_low = "row 0, class %d" % next((c for c in range(4) if not z[c] >= ex.LAW_FLOOR), 0)
            call = (lambda: ex.class_marginals_site(NAME[code], chain, table, lds_width=lds_width)) if site else \
                (lambda: ex.class_marginals(NAME[code], chain, w4=w4, lds_width=lds_width))
            done, res = answered_or_refused(call, not ok, first_low, where)
            outcomes.setdefault("class_marginals", set()).add(done)
            if done:
                for c in range(4):
                    exact = laws[c].marginals()
                    err = worst_error(res["marginals"][0, c].reshape(nq, 4)[cells], [exact[q] for q in cells])
                    worst["class_marginals"] = max(worst.get("class_marginals", 0), err)
                    assert err <= tol, (where, c, float(err))
            else:
                assert want_z[int(first_low.split("class ")[1])] < FLOOR and low <= int(first_low.split("class ")[1])
            done, res = answered_or_refused(lambda: ex.exact_error_counts(NAME[code], chain, p, lds_width=lds_width), not ok, first_low, where)
            outcomes.setdefault("exact_error_counts", set()).add(done)
            if done:
                post = Q.posterior_marginals(laws)
                errs = [abs(Fraction(float(res["per_class"][0, c])) - Q.error_count(laws[c].marginals(), cells)) for c in range(4)]
                errs.append(abs(Fraction(float(res["posterior"][0])) - Q.error_count(post, cells)))
                worst["exact_error_counts"] = max(worst.get("exact_error_counts", 0), max(errs))
                assert max(errs) <= tol * len(cells), (where, [float(e) for e in errs])
        else:
            call = (lambda: ex.posterior_marginals(NAME[code], chain, site_weights=table, lds_width=lds_width)) if site else \
                (lambda: ex.posterior_marginals(NAME[code], chain, w4=w4, lds_width=lds_width))
            done, res = answered_or_refused(call, total < FLOOR, "row 0: the class weights total", where)
            outcomes.setdefault("posterior_marginals", set()).add(done)
            if done:
                exact = Q.posterior_marginals(laws)
                err = worst_error(res[0].reshape(nq, 4)[cells], [exact[q] for q in cells])
                worst["posterior_marginals"] = max(worst.get("posterior_marginals", 0), err)
                assert err <= tol, (where, float(err))
    print("%s L=%d lds_width=%d %s: worst absolute errors %s" % (NAME[code], L, lds_width, kind, {f: "%.3g" % float(v) for f, v in worst.items()}))
    assert seen == {"normal", "subnormal", "zero"}
    assert all(outcomes[f] == {True, False} for f in ("class_marginals", "exact_error_counts", "posterior_marginals")), outcomes


def test_posterior_error_counts_inherits_the_samplers_refusal(T):
    """the function draws through sample_posterior, whose refusal is the library's: the twin refuses the tied row at a total of 1e-320 by name"""
    case = R.rows_of(T, ROTATED, 3)
    w4 = ex.depolarizing_w4(R.ladder(case["least"][0])[280])
    rc, msg, *_ = SA.twin_rc(T, ROTATED, 3, case["chains"][:1], w=w4, K=4, mode=1)
    assert rc == -1 and msg.startswith("qecmc_class_sample: row 0: the class weights total") and "below 2^-960" in msg


# ------------------------------------------------------------------------------------------------------ the top of the range
def test_overflow_is_refused_by_name_in_both_families(T, monkeypatch):
    monkeypatch.setattr(ex, "_marginals", through_the_twin(T, 3))
    chains = R.rows_of(T, ROTATED, 3)["chains"]
    big = np.array([1e120, 1.0, 1.0, 1.0])
    wq = np.broadcast_to(ex.depolarizing_w4(0.1), (2, 9, 4)).copy()
    wq[1, :, 1:] = 1e40
    for mode in (0, 1):
        rc, msg, _, _, z = SA.twin_rc(T, ROTATED, 3, chains, w=big, K=2, mode=mode)
        assert rc == -1 and np.isinf(z[0]).all() and msg.startswith("qecmc_class_sample: row 0" + (", class 0: the class weight is inf" if mode == 0 else ": the class weights total inf"))
        rc, msg, _, _, z = SA.twin_rc(T, ROTATED, 3, chains, wq=wq, K=2, mode=mode)
        assert rc == -1 and np.isfinite(z[0]).all() and np.isinf(z[1]).any() and msg.startswith("qecmc_class_sample_site: row 1") and "inf" in msg
    table = wq.reshape(2, 3, 3, 4)
    raw = ex.class_marginals_site("rotated", chains, table, normalize=False)
    assert not np.isnan(raw["weights"]).any() and np.isinf(raw["z"][1]).any() and np.isfinite(raw["weights"][0]).all()
    with pytest.raises(FloatingPointError, match="row 1, class [0-3]: the class weight is inf"):
        ex.class_marginals_site("rotated", chains, table)
    with pytest.raises(FloatingPointError, match="row 1: the class weights total inf"):
        ex.posterior_marginals("rotated", chains, site_weights=table)
    with pytest.raises(FloatingPointError, match="row 0, class 0: the class weight is inf"):
        ex.class_marginals("rotated", chains, w4=big)
    with pytest.raises(FloatingPointError, match="row 0: the class weights total inf"):
        ex.posterior_marginals("rotated", chains, w4=big)
    assert np.isfinite(ex.class_marginals_site("rotated", chains[:1], table[0])["marginals"]).all()


# ------------------------------------------------------------------------------------------------------ the cases the GPU file runs
def gpu_case_inputs(T, case):
    """(chains uint8[2, ...], w, wq) of a case of sample_range_cases.py"""
    code, L = case[0], case[1]
    rows = R.rows_of(T, code, L)
    w, wq = RC.weights_of(case, {"row": R.ladder(rows["least"][0]), "class": class_ladder(rows, 0)}, ex.depolarizing_w4)
    return rows["chains"], w, wq


def case_id(c):
    return "%s-%d-%d-%s-%d-%s" % ((R.NAME[c[0]],) + tuple(c[1:]))


@pytest.mark.parametrize("case", RC.CASES, ids=case_id)
def test_the_shared_cases_meet_their_premises_on_the_twin(T, case, monkeypatch):
    code, L, lds_width, ladder, step, form = case
    chains, w, wq = gpu_case_inputs(T, case)
    ranges, per_class, per_row = RC.premise_of(case)
    out, z, _ = MA.twin(T, code, L, chains, w=w, wq=wq, lds_width=lds_width)
    assert RC.ranges_of(z[0]) == ranges, (RC.ranges_of(z[0]), z[0])
    for mode, answers in ((0, per_class), (1, per_row)):
        rc, msg, _, _, zs = SA.twin_rc(T, code, L, chains[:1], w=w, wq=None if wq is None else wq[:1] if wq.ndim == 3 else wq, K=2, mode=mode, lds_width=lds_width)
        assert SC_bits(zs) == SC_bits(z[:1])
        assert (rc == 0) == answers and (answers or "row 0" in msg), (mode, msg)
    monkeypatch.setattr(ex, "_marginals", through_the_twin(T, L))
    table = None if wq is None else (wq[0] if wq.ndim == 3 else wq).reshape(state_shape(code, L) + (4,))
    kw = dict(w4=w) if wq is None else dict(site_weights=table)
    for call, answers in ((lambda: ex.posterior_marginals(NAME[code], chains[:1], lds_width=lds_width, **kw), per_row),
                          (lambda: ex.class_marginals(NAME[code], chains[:1], lds_width=lds_width, **kw) if wq is None else
                           ex.class_marginals_site(NAME[code], chains[:1], table, lds_width=lds_width), per_class)):
        try:
            call()
            assert answers
        except FloatingPointError as e:
            assert not answers and "row 0" in str(e)


def SC_bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()
