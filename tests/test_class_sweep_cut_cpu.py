"""The frontier sweep past one LDS state vector (cut-set conditioning), without a GPU: the planner and the twin of csrc/class_sweep_cut.hpp, compiled
by g++ into the host-table test library (qt_class_sweep_cut_info, _ops, _held, _group, qt_class_sweep_cut), and the Python layer around them.

What is pinned: the invariants of the cut plan against the oracle's stencils (held and swept generators partition the table; every swept generator
lives in one slot from before its first qubit to after its last; every qubit is closed once naming its swept generators; peak = width <= lds_width;
the held words are the held generators' Paulis); the cut twin against the uncut twin where both exist, under the weight families and with
w_X != w_Y, and bit for bit where nothing is held; all-ones weights give exactly 2^rank at toric L = 5, xzzx L = 11 and planar L = 7; one toric
L = 5 syndrome against the product of two sector sums written here; Z as a function of the syndrome alone; the refusals by name; resolve_method.

Tolerance against the uncut twin 1e-12 relative per class weight: all terms are positive, either side errs by about (nq + G) 2^-53 < 2e-14, and
1e-12 is what the uncut sweep's tests use.  Against the sector product 1e-10 relative: the sector sums are sums of 2^24 positive terms in NumPy's
pairwise order (error below 24 * 2^-53 relative each), far inside."""
import ctypes as C

import numpy as np
import pytest

import test_class_sweep_cpu as S
from hostlib import run_selftest
from qecmc import _lib as L_
from qecmc import exact as ex
from test_corrections_cpu import classes, generators
from test_enumerate_cpu import class_chains
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape

NAME = S.NAME
INTRO, CLOSE, FORGET = 0, 1, 2
MAX_HELD = 12
_u8p, _u32p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double)
# every accepted (code, L, lds_width) the tests of this file and of tests/test_gpu_class_sweep_cut.py use
ACCEPTED = [(TORIC, 3, 10), (TORIC, 3, 8), (TORIC, 3, 5), (XZZX, 5, 6), (ROTATED, 5, 5), (PLANAR, 3, 3), (XZZX, 3, 0), (ROTATED, 5, 0), (ROTATED, 9, 0),
            (TORIC, 5, 13), (TORIC, 5, 14), (TORIC, 5, 0), (XZZX, 11, 0), (ROTATED, 11, 14), (PLANAR, 7, 0), (PLANAR, 7, 13)]
INFO_KEYS = ("full_width", "width", "held", "ncls", "nq", "n_ops", "rank", "n_gen", "lds_bytes", "max_held", "max_width", "lds_width")


def load_twin():
    """the host-table test library with the cut sweep's entry points (tests/test_gpu_class_sweep_cut.py compares the GPU with it)"""
    lib = S.load_twin()
    lib.qt_class_sweep_cut_info.restype = C.c_int
    lib.qt_class_sweep_cut_info.argtypes = [C.c_int, C.c_int, C.c_int, _i32p, C.c_char_p, C.c_int]
    lib.qt_class_sweep_cut_ops.restype = C.c_int
    lib.qt_class_sweep_cut_ops.argtypes = [C.c_int, C.c_int, C.c_int, _u32p, C.c_int]
    lib.qt_class_sweep_cut_held.restype = C.c_int
    lib.qt_class_sweep_cut_held.argtypes = [C.c_int, C.c_int, C.c_int, _i32p, _u32p, C.c_int]
    lib.qt_class_sweep_cut_group.restype = C.c_uint32
    lib.qt_class_sweep_cut_group.argtypes = [C.c_uint64, C.c_int, C.c_int]
    lib.qt_class_sweep_cut.restype = C.c_int
    lib.qt_class_sweep_cut.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, _f64p, C.c_int, _f64p, _i32p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def info(T, code, L, lds_width):
    """(rc, dict of INFO_KEYS, message)"""
    v, msg = np.zeros(12, np.int32), C.create_string_buffer(512)
    rc = T.qt_class_sweep_cut_info(code, L, lds_width, v.ctypes.data_as(_i32p), msg, 512)
    return rc, dict(zip(INFO_KEYS, v.tolist())), msg.value


def twin(T, code, L, chains, w, lds_width=0):
    """the host twin on chains [N, ...] -> (Z float64[N, ncls], cls int32[N])"""
    nq = int(np.prod(state_shape(code, L)))
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    w = np.ascontiguousarray(w, dtype=np.float64)
    z, cls = np.full((len(flat), 16 if code == TORIC else 4), -1.0), np.full(len(flat), 9, np.int32)
    rc = T.qt_class_sweep_cut(code, L, len(flat), flat.ctypes.data_as(_u8p), w.ctypes.data_as(_f64p), lds_width, z.ctypes.data_as(_f64p), cls.ctypes.data_as(_i32p))
    assert rc == 0, rc
    return z, cls


def ops_of(T, code, L, lds_width):
    """the op stream as test_class_sweep_cpu.ops_of gives it"""
    _, inf, _ = info(T, code, L, lds_width)
    buf = np.zeros(4 * inf["n_ops"], np.uint32)
    assert T.qt_class_sweep_cut_ops(code, L, lds_width, buf.ctypes.data_as(_u32p), buf.size) == buf.size
    out = []
    for w0, mask, pairs, qubit in buf.reshape(-1, 4).tolist():
        pr = [((pairs >> 8 * j) & 15, (pairs >> (8 * j + 4)) & 15) for j in range((w0 >> 8) & 15)]
        out.append((w0 & 15, (w0 >> 4) & 15, (w0 >> 12) & 31, mask, [(s, xz ^ (xz >> 1)) for s, xz in pr], qubit))
    return out


def held_of(T, code, L, lds_width):
    """(table indices int32[n_held], the held generators as byte chains uint8[n_held, nq])"""
    _, inf, _ = info(T, code, L, lds_width)
    W = (inf["nq"] + 15) // 16
    index, words = np.full(MAX_HELD, -1, np.int32), np.zeros(MAX_HELD * W, np.uint32)
    n = T.qt_class_sweep_cut_held(code, L, lds_width, index.ctypes.data_as(_i32p), words.ctypes.data_as(_u32p), words.size)
    assert n == inf["held"]
    words = words[:n * W].reshape(n, W)
    q = np.arange(inf["nq"])
    return index[:n], ((words[:, q >> 4] >> ((q & 15) * 2).astype(np.uint32)) & 3).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("code,L,lds_width", ACCEPTED)
def test_cut_plan_invariants(T, code, L, lds_width):
    rc, inf, msg = info(T, code, L, lds_width)
    assert rc == 0, msg
    gens = generators(code, L)
    print("%s L=%d lds_width %d: full width %d, held %d, width %d, %d ops" % (NAME[code], L, lds_width, inf["full_width"], inf["held"], inf["width"], inf["n_ops"]))
    assert inf["max_held"] == MAX_HELD and inf["max_width"] == 14 and inf["held"] <= MAX_HELD
    assert inf["width"] <= inf["lds_width"] <= 14 and (lds_width == 0 or inf["lds_width"] == lds_width)
    assert inf["lds_bytes"] == 8 << inf["width"] <= 128 * 1024
    assert inf["full_width"] == S.info(T, code, L)[1]["width"]                  # the uncut planner's, also where that one refuses the width
    assert inf["held"] >= inf["full_width"] - inf["lds_width"] and (inf["held"] == 0) == (inf["full_width"] <= inf["lds_width"])
    assert inf["n_gen"] == len(gens) and inf["rank"] == (len(gens) - 2 if code == TORIC else len(gens))
    index, held = held_of(T, code, L, lds_width)
    assert len(set(index.tolist())) == len(index) and np.all(np.diff(index) > 0) and np.all((index >= 0) & (index < len(gens)))
    assert np.array_equal(held, gens[index])                                    # held_words[j] is generator index[j]'s Paulis
    swept = [g for g in range(len(gens)) if g not in set(index.tolist())]       # held and swept: disjoint, and together the table
    sw = gens[swept]
    live, lifetimes, closed, peak = {}, [], [], 0
    for kind, slot, top, mask, pairs, qubit in ops_of(T, code, L, lds_width):
        before = sum(1 << s for s in live)
        if kind == INTRO:
            assert slot not in live and mask == before and top > slot and mask >> top == 0
            live[slot] = set()
            peak = max(peak, len(live))
        elif kind == CLOSE:
            assert mask == before and mask >> top == 0 and len({s for s, _ in pairs}) == len(pairs)
            for s, pauli in pairs:
                assert s in live and pauli in (1, 2, 3)
                live[s].add((qubit, pauli))
            closed.append(qubit)
            assert sorted(p for _, p in pairs) == sorted(int(g[qubit]) for g in sw if g[qubit])        # exactly its generators that are not held
        else:
            assert kind == FORGET and slot in live and top > slot
            lifetimes.append(frozenset(live.pop(slot)))
            assert mask == sum(1 << s for s in live) and mask >> top == 0
    assert not live and peak == inf["width"]
    assert sorted(closed) == [q for q in range(gens.shape[1]) if gens[:, q].any()]      # every qubit once, also one only held generators touch
    supports = [frozenset((q, int(g[q])) for q in np.flatnonzero(g)) for g in sw]
    assert sorted(map(sorted, lifetimes)) == sorted(map(sorted, supports))      # one lifetime per swept generator, covering exactly its qubits


def test_what_the_planner_holds(T):
    """the planner's own numbers (DESIGN.md 4.1l has the table): toric L = 5 fits width 13 with 8 held generators and width 14 with 7; the width-14
    shapes hold nothing by default; a shape the uncut sweep takes holds nothing by default"""
    got = {(NAME[c], L, w): tuple(info(T, c, L, w)[1][k] for k in ("full_width", "held", "width")) for c, L, w in ACCEPTED}
    print(got)
    assert got["toric", 5, 13] == (21, 8, 13) and got["toric", 5, 14] == (21, 7, 14) and got["toric", 5, 0] in (got["toric", 5, 13], got["toric", 5, 14])
    assert got["xzzx", 11, 0] == (14, 0, 14) and got["rotated", 11, 14] == (14, 0, 14) and got["planar", 7, 0] == (14, 0, 14)
    assert got["rotated", 9, 0][1] == 0 and got["xzzx", 3, 0][1] == 0
    assert got["toric", 3, 5][1:] == (8, 5) and got["planar", 7, 13][2] == 13 and got["planar", 7, 13][1] >= 1


def test_launch_groups(T):
    """one launch of the sweep kernel stays within 2^16 workgroups and 1 024 syndromes"""
    for ncls in (4, 16):
        for held in range(MAX_HELD + 1):
            for n in (0, 1, 7, 1 << 20):
                g = T.qt_class_sweep_cut_group(n, ncls, held)
                assert 1 <= g <= 1024 and (g * ncls << held) <= 1 << 16 and (n == 0 or g <= n), (ncls, held, n, g)
    assert T.qt_class_sweep_cut_group(1 << 20, 16, 5) == 128 and T.qt_class_sweep_cut_group(1 << 20, 4, 0) == 1024


# ------------------------------------------------------------------------------------------------------ the twin against the uncut twin
@pytest.mark.parametrize("code,L,lds_width", [(TORIC, 3, 10), (TORIC, 3, 8), (TORIC, 3, 5), (XZZX, 5, 6), (ROTATED, 5, 5), (PLANAR, 3, 3)])
def test_cut_twin_is_the_uncut_twin(T, code, L, lds_width):
    rc, inf, _ = info(T, code, L, lds_width)
    assert rc == 0 and inf["held"] >= 1 and inf["width"] <= lds_width
    chains = random_errors(code, L, 3, np.random.default_rng([31, code, L]))
    families = ([ex.depolarizing_w4(0.1), ex.depolarizing_w4(0.2), ex.depolarizing_w4(0.4)] if code == TORIC else
                [ex.depolarizing_w4(0.1), ex.biased_w4(0.25, 3.0), ex.alpha_w4(0.3, 2.5)]) + [S.SKEW]
    for w4 in families:
        z, cls = twin(T, code, L, chains, w4, lds_width)
        want, wcls = S.twin(T, code, L, chains, w4)
        print(NAME[code], L, lds_width, "max relative difference %.3g" % S.rel(z, want).max())
        assert S.rel(z, want).max() < 1e-12 and np.array_equal(cls, wcls) and np.array_equal(cls, classes(code, chains))
    swapped, _ = twin(T, code, L, chains, S.SKEW[[0, 2, 1, 3]], lds_width)
    assert S.rel(swapped, S.twin(T, code, L, chains, S.SKEW)[0]).max() > 1e-3     # (the case tells X from Y)


@pytest.mark.parametrize("code,L,lds_width", [(XZZX, 3, 0), (ROTATED, 5, 0), (TORIC, 3, 13), (PLANAR, 4, 14), (ROTATED, 7, 10)])
def test_with_nothing_held_the_cut_twin_is_the_uncut_twin_bit_for_bit(T, code, L, lds_width):
    assert info(T, code, L, lds_width)[1]["held"] == 0
    chains = random_errors(code, L, 3, np.random.default_rng([32, code, L]))
    z, cls = twin(T, code, L, chains, S.SKEW, lds_width)
    want, wcls = S.twin(T, code, L, chains, S.SKEW)
    assert np.array_equal(z.view(np.uint64), want.view(np.uint64)) and np.array_equal(cls, wcls)
    buf = np.zeros(4 * S.info(T, code, L)[1]["n_ops"], np.uint32)
    assert T.qt_class_sweep_ops(code, L, buf.ctypes.data_as(_u32p), buf.size) == buf.size
    cut = np.zeros_like(buf)
    assert T.qt_class_sweep_cut_ops(code, L, lds_width, cut.ctypes.data_as(_u32p), cut.size) == cut.size and np.array_equal(cut, buf)


@pytest.mark.parametrize("code,L,lds_width", [(TORIC, 5, 13), (XZZX, 11, 0), (PLANAR, 7, 0)])
def test_all_ones_weights_count_the_group(T, code, L, lds_width):
    """w = (1, 1, 1, 1): every class weight is 2^rank exactly -- 2^48 on the torus at L = 5 after the division by 4 --: sums of equal powers of two"""
    _, inf, _ = info(T, code, L, lds_width)
    chains = random_errors(code, L, 1, np.random.default_rng([5, code, L]))
    z, _ = twin(T, code, L, chains, np.ones(4), lds_width)
    assert inf["rank"] == {TORIC: 2 * L * L - 2, PLANAR: 2 * L * (L - 1)}.get(code, L * L - 1) and (code != TORIC or inf["rank"] == 48)
    assert np.all(z == 2.0 ** inf["rank"])


# ------------------------------------------------------------------------------------------------------ toric L = 5 against an independent computation
def sector_sums(gens, chain, f):
    """For a weight with w_Y = w_X w_Z the weight of a chain is f_x^(its X-or-Y count) f_z^(its Z-or-Y count), and the torus' vertex generators (all X)
    and plaquette generators (all Z) move the two counts independently: Z = S_x S_z / 4, S_x = the sum over all 2^25 subsets of the X-type generators of
    f_x^(X-or-Y count), S_z likewise -- every group element is met twice in either sector.  Each by brute force over the bit planes, 2^25 terms."""
    out = []
    for bit, fs in ((0, f[0]), (1, f[1])):                                     # byte values: X = 1 = 0b01, Z = 3 = 0b11, Y = 2 = 0b10; x part: 1 or 2, z part: 2 or 3
        part = (lambda a: ((a == 1) | (a == 2))) if bit == 0 else (lambda a: (a >= 2))
        mine = [g for g in gens if (g == (1, 3)[bit]).any()]
        assert len(mine) == 25 and all(set(np.unique(g).tolist()) == {0, (1, 3)[bit]} for g in mine)     # the sector's generators are of one Pauli
        rows = np.array([sum(1 << int(q) for q in np.flatnonzero(part(g))) for g in mine], dtype=np.uint64)
        start = np.uint64(sum(1 << int(q) for q in np.flatnonzero(part(chain))))
        lo = np.zeros(1, np.uint64)                                             # the XORs of the subsets of the first 16 rows, and of the other 9
        for r in rows[:16]:
            lo = np.concatenate([lo, lo ^ r])
        hi = np.zeros(1, np.uint64)
        for r in rows[16:]:
            hi = np.concatenate([hi, hi ^ r])
        pw = fs ** np.arange(51, dtype=np.float64)
        total = 0.0
        for h in hi:
            v = lo ^ (h ^ start)
            cnt = np.zeros(v.shape, np.int64)
            for k in range(0, 64, 16):
                cnt += _POP16[((v >> np.uint64(k)) & np.uint64(0xFFFF)).astype(np.int64)]
            total += pw[cnt].sum()
        out.append(total)
    return out[0] * out[1] / 4.0


_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.int64)


def test_toric_L5_is_the_product_of_its_two_sector_sums(T):
    """one random syndrome at p = 0.15, three classes, under weights with w_Y = w_X w_Z and w_X != w_Z (fx = 0.15 / 0.85 as the error rate, fz half of
    it): the cut sweep at width 13 (8 held) against brute force over the X-type and the Z-type generators separately"""
    rng = np.random.default_rng(515)
    chain = np.zeros((2, 5, 5), np.uint8)
    err = rng.random(chain.shape) < 0.15
    chain[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    fx, fz = 0.15 / 0.85, 0.075 / 0.85
    w4 = np.array([1.0, fx, fx * fz, fz])
    z, cls = twin(T, TORIC, 5, chain[None], w4, 13)
    gens = generators(TORIC, 5)
    reps = class_chains(TORIC, chain)
    for c in (int(cls[0]), (int(cls[0]) + 5) % 16, (int(cls[0]) + 10) % 16):
        want = sector_sums(gens, reps[c].reshape(-1), (fx, fz))
        print("class %d: cut sweep %.17g, sector product %.17g, relative difference %.3g" % (c, z[0, c], want, abs(z[0, c] - want) / want))
        assert abs(z[0, c] - want) / want < 1e-10
    z14, _ = twin(T, TORIC, 5, chain[None], w4, 14)
    assert S.rel(z14, z).max() < 1e-12                                          # (7 held at width 14: another split of the same sum)


# ------------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("code,L,lds_width", [(TORIC, 3, 8), (XZZX, 5, 6), (TORIC, 5, 14)])
def test_Z_is_a_function_of_the_syndrome(T, code, L, lds_width):
    chains = random_errors(code, L, 1 if L == 5 and code == TORIC else 3, np.random.default_rng([6, code, L]))
    z, cls = twin(T, code, L, chains, S.SKEW, lds_width)
    assert np.array_equal(cls, classes(code, chains))
    gens, rng = generators(code, L), np.random.default_rng([7, code, L])
    moved = chains.copy()
    for s in range(len(moved)):
        for g in rng.integers(len(gens), size=7):
            moved[s] ^= gens[g].reshape(moved[s].shape)
    ncls = z.shape[1]
    other = np.stack([class_chains(code, m)[(c + 1) % ncls].reshape(m.shape) for m, c in zip(moved, cls)])   # and a logical operator away
    z2, c2 = twin(T, code, L, other, S.SKEW, lds_width)
    assert S.rel(z2, z).max() < 1e-12 and np.array_equal(c2, (cls + 1) % ncls)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(T):
    for code, L, w in [(XZZX, 4, 0), (TORIC, 1, 0), (TORIC, 65, 13), (-1, 3, 0), (4, 3, 0)]:
        assert info(T, code, L, w)[0] == -1, (code, L, w)
    for w in (1, 15, -1, 99):
        rc, _, msg = info(T, XZZX, 3, w)
        assert rc == -1 and b"lds_width" in msg, (w, msg)
    for code, L, w, frags in [(TORIC, 4, 0, [b"even length"]), (TORIC, 7, 0, [b"held generators", b"29 generators wide", b"12 held"]),
                              (TORIC, 7, 14, [b"held generators"]), (PLANAR, 8, 0, [b"held generators", b"16 generators wide"]),
                              (ROTATED, 13, 0, [b"held generators", b"16 generators wide"]), (XZZX, 13, 14, [b"held generators"]),
                              (TORIC, 63, 0, [b"held generators"]), (PLANAR, 64, 0, [b"held generators"])]:
        rc, inf, msg = info(T, code, L, w)
        print(NAME[code], L, w, msg)
        assert rc == -4 and all(f in msg for f in frags), (code, L, w, msg)
    # the uncut entry points answer what they answered
    for code, L, frag in [(TORIC, 5, b"21 generators wide"), (XZZX, 11, b"14 generators wide"), (PLANAR, 7, b"14 generators wide")]:
        rc, _, msg = S.info(T, code, L)
        assert rc == -4 and frag in msg and b"65536 bytes" in msg and b"width 13 at most" in msg
    chains, z = np.zeros((1, 9), np.uint8), np.zeros((1, 4))
    call = lambda w, c=chains, out=z, lw=0: T.qt_class_sweep_cut(XZZX, 3, 1, None if c is None else c.ctypes.data_as(_u8p),
                                                                 None if w is None else np.array(w, np.float64).ctypes.data_as(_f64p), lw,
                                                                 None if out is None else out.ctypes.data_as(_f64p), None)
    assert call([1, 1, 1, 1]) == 0
    for bad in ([1, 0, 1, 1], [1, 1, -0.5, 1], [1, 1, 1, np.nan], [np.inf, 1, 1, 1]):
        assert call(bad) == -1, bad
    assert call(None) == -1 and call([1, 1, 1, 1], c=None) == -1 and call([1, 1, 1, 1], out=None) == -1
    assert call([1, 1, 1, 1], lw=1) == -1 and call([1, 1, 1, 1], lw=15) == -1


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    chains, z, cls = np.zeros((1, 9), np.uint8), np.zeros((1, 4)), np.zeros(1, np.int32)
    big = np.zeros((1, 2 * 13 * 13), np.uint8)
    zp = z.ctypes.data_as(_f64p)
    wp = lambda w: np.array(w, np.float64).ctypes.data_as(_f64p)
    ones = wp([1, 1, 1, 1])
    cut = lib.qecmc_class_sweep_cut
    assert cut(XZZX, 3, 1, None, ones, 0, zp, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert cut(XZZX, 3, 1, L_.u8(chains), None, 0, zp, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert cut(XZZX, 3, 1, L_.u8(chains), ones, 0, None, None) == -1 and b"NULL" in lib.qecmc_last_error()
    for bad in ([1, 0, 1, 1], [1, 1, -1, 1], [1, 1, 1, np.nan], [1, np.inf, 1, 1]):
        assert cut(XZZX, 3, 1, L_.u8(chains), wp(bad), 0, zp, None) == -1 and b"finite and > 0" in lib.qecmc_last_error()
    assert cut(XZZX, 4, 1, L_.u8(chains), ones, 0, zp, None) == -1 and b"odd L" in lib.qecmc_last_error()
    assert cut(7, 3, 1, L_.u8(chains), ones, 0, zp, None) == -1 and b"code" in lib.qecmc_last_error()
    for w in (1, 15, -3):
        assert cut(XZZX, 3, 1, L_.u8(chains), ones, w, zp, None) == -1 and b"lds_width" in lib.qecmc_last_error()
    assert cut(TORIC, 4, 1, L_.u8(big), ones, 0, zp, None) == -4 and b"even length" in lib.qecmc_last_error()
    assert cut(TORIC, 7, 1, L_.u8(big), ones, 0, zp, None) == -4 and b"held generators" in lib.qecmc_last_error()
    assert cut(PLANAR, 8, 1, L_.u8(big), ones, 14, zp, None) == -4 and b"held generators" in lib.qecmc_last_error()
    assert cut(ROTATED, 13, 1, L_.u8(big), ones, 0, zp, None) == -4 and b"held generators" in lib.qecmc_last_error()
    # the entry points of before still answer -4 at toric L = 5
    assert lib.qecmc_class_sweep(TORIC, 5, 1, L_.u8(big), ones, zp, None) == -4 and b"21 generators wide" in lib.qecmc_last_error()
    assert lib.qecmc_class_sweep_info(TORIC, 5, None, None, None, None) == -4
    assert lib.qecmc_coset_enumerate_info(TORIC, 5, None, None, None, None) == -4
    assert lib.qecmc_abi_version() == 4
    v = [C.c_int32() for _ in range(6)]
    assert lib.qecmc_class_sweep_cut_info(TORIC, 5, 14, *[C.byref(x) for x in v]) == 0 and [x.value for x in v] == [21, 14, 7, 16, 50, v[5].value]
    assert lib.qecmc_class_sweep_cut_info(TORIC, 5, 0, None, None, None, None, None, None) == 0
    assert lib.qecmc_class_sweep_cut_info(TORIC, 7, 0, None, None, None, None, None, None) == -4
    assert ex.sweep_cut_info("toric", 5, 13) == dict(full_width=21, width=13, held=8, ncls=16, nq=50, n_ops=ex.sweep_cut_info("toric", 5, 13)["n_ops"])
    assert ex.sweep_cut_info("planar", 7)["held"] == 0 and ex.sweep_cut_info("rotated", 9)["width"] == ex.sweep_info("rotated", 9)["width"]
    # a valid call gets as far as the device lookup: no device, no CPU fallback
    have = L_.device_count() >= 1
    for n in (1, 0):
        assert cut(XZZX, 3, n, L_.u8(chains), ones, 0, zp, L_.i32(cls)) == (0 if have else -2)
    if not have:
        assert b"no CPU fallback" in lib.qecmc_last_error()
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.class_sweep_cut("xzzx", chains.reshape(1, 3, 3), np.ones(4))
    with pytest.raises(ValueError, match="four weights"):
        ex.class_sweep_cut("xzzx", chains.reshape(1, 3, 3), np.ones(3))
    with pytest.raises(L_.QecmcError, match="lds_width"):
        ex.class_sweep_cut("xzzx", chains.reshape(1, 3, 3), np.ones(4), lds_width=15)


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_auto_is_the_cut_sweep_where_enumerator_and_sweep_both_refuse(T):
    for code, L in [(TORIC, 5), (XZZX, 11), (ROTATED, 11), (PLANAR, 7)]:
        assert ex.resolve_method(NAME[code], L) == "cut" and ex.resolve_method(code, L) == "cut"
    # everything of before is unchanged
    import test_enumerate_cpu as E
    for code, L in E.SUPPORTED:
        assert ex.resolve_method(NAME[code], L) == "enumerate" and ex.resolve_method(code, L, "sweep") == "sweep" and ex.resolve_method(code, L, "cut") == "cut"
    for code, L in [(XZZX, 7), (XZZX, 9), (ROTATED, 7), (ROTATED, 9), (PLANAR, 5), (PLANAR, 6)]:
        assert ex.resolve_method(NAME[code], L) == "sweep"
    assert ex.resolve_method("xzzx", 4) == "enumerate"
    for code, L in [(TORIC, 4), (TORIC, 7), (PLANAR, 8), (ROTATED, 13)]:         # (refused by all three: the sweep's refusal is the one to report, as before)
        assert ex.resolve_method(NAME[code], L) == "sweep"
    with pytest.raises(ValueError):
        ex.resolve_method("toric", 5, "best")
    with pytest.raises(ValueError, match="chunks"):
        ex.exact_class_probabilities("toric", np.zeros((1, 2, 5, 5), np.uint8), 0.1, chunks=(0, 1))


# ------------------------------------------------------------------------------------------------------ the sanitizers
def test_cut_sweep_under_sanitizers():
    """a stand-alone program (its own main) built from class_sweep_cut.hpp with -fsanitize=address,undefined: cut plans of every (code, L) up to 13,
    accepted or refused, under several widths, and the twin -- threaded and not -- against the uncut twin; run as a child process"""
    run_selftest("sweep_cut_asan", "class_sweep_cut_selftest_asan")
