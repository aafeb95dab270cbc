"""The host side of libqecmc under test and under sanitizers (SURVEY.md 5 "-fsanitize=address on host lib"):
every table the plan precomputes for the kernels -- generator tables, logical-operator masks, acceptance / swap thresholds,
ladder temperatures, the biased rules' power and count-change tables, the colour phases of scan = 2 -- is built by
csrc/tables.hpp and put together into a plan by csrc/plan_host.hpp, both compiled here ALONE by g++ (no HIP, no GPU); the tables are
compared with values the oracle computes.  The last test
re-runs this file in a child process against the -fsanitize=address,undefined build."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from qecmc import _lib as L_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc")
TORIC, XZZX, ROTATED, PLANAR = 0, 1, 2, 3
ORC_CODE = {TORIC: orc.TORIC, XZZX: orc.XZZX, ROTATED: orc.ROTATED, PLANAR: orc.PLANAR}
SHAPES = [(TORIC, 3), (TORIC, 4), (TORIC, 9), (TORIC, 15), (XZZX, 3), (XZZX, 9), (ROTATED, 5), (ROTATED, 21), (PLANAR, 4), (PLANAR, 9)]


@pytest.fixture(scope="module")
def T():
    path = os.environ.get("QECMC_TABLES_LIB")
    if not path:
        subprocess.check_call(["make", "-C", CSRC, "-s", "tables"])
        path = os.path.join(CSRC, "build", "libqecmc_tables.so")
    lib = C.CDLL(path)
    lib.qt_thr64.restype = C.c_uint64; lib.qt_thr64.argtypes = [C.c_double]
    lib.qt_thr44.restype = C.c_uint64; lib.qt_thr44.argtypes = [C.c_double]
    lib.qt_thr32.restype = C.c_uint32; lib.qt_thr32.argtypes = [C.c_double]
    lib.qt_chain_factor.restype = C.c_double; lib.qt_chain_factor.argtypes = [C.c_double]
    lib.qt_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.qt_plan_key_equal.argtypes = lib.qt_plan_equal.argtypes = [C.c_void_p, C.c_void_p]
    lib.qt_workspace_need.restype = C.c_uint64; lib.qt_workspace_need.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_int]
    return lib


def _nq(code, L):
    return 2 * L * L if code in (TORIC, PLANAR) else L * L


def _zero(code, L):
    return np.zeros((2, L, L) if code in (TORIC, PLANAR) else (L, L), np.uint8)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _gen_table(T, code, L):
    buf = np.zeros(4 * 4096, np.uint32)
    n = T.qt_generator_table(code, L, _ptr(buf, C.c_uint32), buf.size)
    assert n > 0 and n % 2 == 0
    e = buf[:n].view(np.uint16).reshape(n // 2, 4)                     # 4 x (site << 2 | pauli) per generator, 0 = no site
    return e


def _oracle_generator(code, L, g):
    if code == TORIC:
        return orc.toric_apply_stabilizer(_zero(code, L), (g % (L * L)) // L, g % L, 1 if g < L * L else 3)[0].ravel()
    return orc.surf_apply_stabilizer(ORC_CODE[code], _zero(code, L), *orc.surf_gen_rco(ORC_CODE[code], L, g))[0].ravel()


@pytest.mark.parametrize("code,L", SHAPES)
def test_generator_table_is_the_oracles_stencil(T, code, L):
    e = _gen_table(T, code, L)
    G = 2 * L * L if code == TORIC else orc.surf_ngen(ORC_CODE[code], L)
    assert e.shape[0] == G
    for g in range(G):
        pat = np.zeros(_nq(code, L), np.uint8)
        for ent in e[g]:
            if ent:
                assert ent & 3 and pat[ent >> 2] == 0                    # a real site carries a Pauli and appears once
                pat[ent >> 2] = ent & 3
        assert np.array_equal(pat, _oracle_generator(code, L, g)), g


@pytest.mark.parametrize("code,L", SHAPES)
def test_logical_masks_are_the_oracles_operators(T, code, L):
    nq = _nq(code, L); W = (nq + 15) // 16
    buf = np.zeros(4 * (L + 1) * W, np.uint32)
    assert T.qt_logical_masks(code, L, W, _ptr(buf, C.c_uint32), buf.size) == buf.size
    m = buf.reshape(4, L + 1, W)
    unpack = lambda words: np.array([(int(words[q >> 4]) >> ((q & 15) * 2)) & 3 for q in range(nq)], np.uint8)
    z = _zero(code, L)
    for pos in range(L):
        if code == TORIC:
            want = [orc.toric_apply_logical(z, 1, 0, pos, 0)[0], orc.toric_apply_logical(z, 3, 0, 0, pos)[0],
                    orc.toric_apply_logical(z, 1, 1, pos, 0)[0], orc.toric_apply_logical(z, 3, 1, 0, pos)[0]]
        else:
            # X alone / Z alone: xzzx op 1 / 3 (xzzx_model.py:291-311), rotated and planar op 1 / 2 (rotated_surface_model.py:260-280)
            oc = ORC_CODE[code]
            want = [orc.surf_apply_logical(oc, z, 1, pos, 0)[0], orc.surf_apply_logical(oc, z, 3 if code == XZZX else 2, 0, pos)[0]]
        for kind, w in enumerate(want):
            assert np.array_equal(unpack(m[kind, pos]), np.asarray(w).ravel()), (kind, pos)
    assert not m[:, L].any()                                             # row L = identity
    if code != TORIC:
        assert not m[2:].any()


def test_thresholds_decide_like_the_floating_point_test(T):
    """u < v with u = x 2^-32 (or 2^-44) must be exactly x < thr(v): the kernels' integer tests against the oracle's double compare"""
    rng = np.random.default_rng(0)
    vs = np.concatenate([rng.random(300), 10.0 ** rng.uniform(-14, 0, 300), [0.0, 1.0, 1.5, 0.5, 2.0 ** -32, 2.0 ** -44, 1 - 2.0 ** -33]])
    for v in vs:
        t64, t44, t32 = T.qt_thr64(float(v)), T.qt_thr44(float(v)), T.qt_thr32(float(v))
        for x in [0, 1, t64 - 1, t64, t64 + 1, 2 ** 32 - 1] + rng.integers(0, 2 ** 32, 8).tolist():
            if 0 <= x < 2 ** 32:
                assert (x < t64) == (x / 2.0 ** 32 < v), (v, x)
        for x in [0, 1, t44 - 1, t44, t44 + 1, 2 ** 44 - 1] + rng.integers(0, 2 ** 44, 8).tolist():
            if 0 <= x < 2 ** 44:
                assert (x < t44) == (x / 2.0 ** 44 < v), (v, x)
        assert t32 == min(t64, 2 ** 32 - 1)
    assert T.qt_chain_factor(0.15) == (0.15 / 3.0) / (1.0 - 0.15)


@pytest.mark.parametrize("p,Nc,eta", [(0.15, 8, None), (0.1, 5, None), (0.18, 15, None), (0.05, 1, None), (0.15, 8, 100.0), (0.2, 3, 3.0)])
def test_ladder_temperatures_and_swap_thresholds(T, p, Nc, eta):
    pl, pd = np.zeros(Nc), np.zeros(max(Nc - 1, 1))
    p_top = 0.75 if eta is None else (eta + 1) / (2 * eta + 1)
    assert T.qt_ladder(C.c_double(p), C.c_double(p_top), Nc, _ptr(pl, C.c_double), _ptr(pd, C.c_double)) == Nc - 1
    code = orc.TORIC if eta is None else orc.XZZX
    ld = orc.Ladder(code, _zero(TORIC if eta is None else XZZX, 3), p, Nc, 0.5, noise=orc.DEPOLARIZING if eta is None else orc.BIASED, eta=eta or 0.0)
    assert np.array_equal(pl, ld.p_ladder)                               # np.linspace(p, p_top, Nc), mcmc.py:65
    if Nc > 1:
        assert np.array_equal(pd[:Nc - 1], ld.p_diff)                    # mcmc.py:69
        nq = 18
        sw = np.zeros((Nc - 1) * (nq + 1), np.uint64)
        assert T.qt_swap_thresholds(_ptr(pd, C.c_double), Nc - 1, nq, _ptr(sw, C.c_uint64), sw.size) == sw.size
        for i in range(Nc - 1):
            for d in range(nq + 1):
                v = math.pow(pd[i], d)                                   # mcmc.py:149 `rel_p ** (ne_hi - ne_lo)`
                assert int(sw[i * (nq + 1) + d]) == (2 ** 32 if v >= 1 else math.ceil(v * 2.0 ** 32))


@pytest.mark.parametrize("alpha_model,p,par,nq", [(0, 0.15, 100.0, 81), (0, 0.3, 3.0, 9), (1, 0.1, 1.7, 25), (1, 0.4, 0.8, 49)])
def test_power_tables_of_the_biased_and_alpha_rules(T, alpha_model, p, par, nq):
    t = np.zeros(4 * (nq + 1))
    assert T.qt_bias_tables(alpha_model, C.c_double(p), C.c_double(par), nq, _ptr(t, C.c_double), t.size) == t.size
    if alpha_model:                                                      # mcmc_alpha.py:31-36
        pt = p + 2 * math.pow(p, par); pp = pt / (1 + pt)
        pz, px = p * (1 - pp), math.pow(p, par) * (1 - pp)
    else:                                                                # mcmc_biased.py:25-27
        pz, px = p * par / (par + 1), p / (2 * (par + 1))
    py = px; pi = 1 - px - py - pz
    for k, base in enumerate((px, py, pz, pi)):
        assert np.array_equal(t[k * (nq + 1):(k + 1) * (nq + 1)], [math.pow(base, n) for n in range(nq + 1)])


@pytest.mark.parametrize("code,L", [(XZZX, 5), (ROTATED, 7), (PLANAR, 5), (TORIC, 5)])
def test_pauli_patterns_and_count_change_table(T, code, L):
    e = _gen_table(T, code, L)
    G = e.shape[0]
    gt = np.zeros(G, np.uint8); pat = np.zeros(32, np.uint32)
    n = T.qt_patterns(code, L, _ptr(gt, C.c_uint8), G, _ptr(pat, C.c_uint32), pat.size)
    assert 0 < n <= 16
    for g in range(G):
        assert int(pat[gt[g]]) == sum(int(e[g, u] & 3) << (2 * u) for u in range(4))
    assert len(set(pat[:n].tolist())) == n
    lut = np.zeros(256 * n, np.uint32)
    assert T.qt_count_change(_ptr(pat, C.c_uint32), n, _ptr(lut, C.c_uint32), lut.size) == lut.size
    for t in range(n):
        for F in range(256):
            old = [(F >> (2 * u)) & 3 for u in range(4)]
            new = [o ^ ((int(pat[t]) >> (2 * u)) & 3) for u, o in enumerate(old)]
            d = [new.count(v) - old.count(v) for v in range(4)]
            assert int(lut[256 * t + F]) == (d[1] + (d[3] << 10) + ((d[1] + d[2]) << 20)) % 2 ** 32


@pytest.mark.parametrize("code,L", SHAPES)
def test_colour_phases_equal_the_oracles(T, code, L):
    buf = np.zeros(64 * 64, np.uint16)
    n = T.qt_colour_phases(code, L, _ptr(buf, C.c_uint16), buf.size)
    mine = buf[:n * 64].reshape(n, 64).astype(np.int32)
    mine[mine == 0xFFFF] = -1
    assert np.array_equal(mine, orc.colour_phases(ORC_CODE[code], L))   # two independent statements of the rule


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("code,L", SHAPES + [(TORIC, 16), (XZZX, 21)])
def test_wave_descriptors_are_the_oracles_stencil(T, code, L):
    """scan = 3's per-generator descriptors (csrc/tables.hpp wave_descriptors), interpreted the way csrc/ladder_wu.hpp does -- fields
    by word / shift, the byte table behind v_perm_b32, the sum of its bytes, the xor values -- against the oracle's stabilizer on
    random packed states: new configuration and error-count change."""
    nq = _nq(code, L)
    W = (nq + 15) // 16
    buf = np.zeros(16 * 4096, np.uint32)
    n = T.qt_wave_descriptors(code, L, _ptr(buf, C.c_uint32), buf.size)
    G = 2 * L * L if code == TORIC else orc.surf_ngen(ORC_CODE[code], L)
    assert n == 16 * G
    d = buf[:n].reshape(G, 16)
    rng = np.random.default_rng(L * 5 + code)
    for g in rng.permutation(G)[:40]:
        m = rng.integers(0, 4, size=_zero(code, L).shape).astype(np.uint8)
        if code == PLANAR:
            m[1, -1, :] = 0; m[1, :, -1] = 0
        flat = m.ravel()
        words = np.zeros(W, np.uint64)
        for q in range(nq):
            words[q >> 4] |= np.uint64(int(flat[q]) << (2 * (q & 15)))
        e = d[g]
        sel = 0
        for i in range(4):
            wi, sh = int(e[i]) & 0xFF, (int(e[i]) >> 8) & 31
            assert wi < W
            sel |= ((int(words[wi]) >> sh) & 0xFF) << (8 * i)              # v_lshrrev_b32_sdwa: a byte, junk above the field
        sel0 = sel
        sel = (sel & int(e[11])) | int(e[10]) if code != TORIC else sel & 0x03030303
        tab = int(e[8]).to_bytes(4, "little") + int(e[9]).to_bytes(4, "little")   # v_perm_b32: selectors 0-3 -> dword 8, 4-7 -> dword 9
        if code == TORIC:
            assert e[8] == e[9]
        dE4 = sum(tab[(sel >> (8 * i)) & 0xFF] for i in range(4))          # v_sad_u8: 4 (dE + 4)
        for i in range(4):
            words[int(e[i]) & 0xFF] ^= np.uint64(int(e[4 + i]))
        new = np.array([(int(words[q >> 4]) >> (2 * (q & 15))) & 3 for q in range(nq)], np.uint8).reshape(m.shape)
        if code == TORIC:
            ref, dE = orc.toric_apply_stabilizer(m, (int(g) % (L * L)) // L, int(g) % L, 1 if g < L * L else 3)
        else:
            ref, dE = orc.surf_apply_stabilizer(ORC_CODE[code], m, *orc.surf_gen_rco(ORC_CODE[code], L, int(g)))
        assert np.array_equal(new, ref)
        assert dE4 == 4 * (dE + 4)
        # dwords 12-15, the alpha rule: the same selector with the missing sites' bytes 0x0C (the constant 0), the byte tables of
        # 4 ((dz + 1) + 9 (dxy + 1)); their sum + dword 15 = the byte offset of (D_xy, D_z) in the kernel's 9 x 9 table
        sel_a = (sel0 & int(e[11])) | int(e[14])
        tab_a = int(e[12]).to_bytes(4, "little") + int(e[13]).to_bytes(4, "little")
        off = int(e[15])
        for i in range(4):
            b = (sel_a >> (8 * i)) & 0xFF
            off += 0 if b == 0x0C else tab_a[b]
        dz = int(np.sum(ref == 3)) - int(np.sum(m == 3))
        dxy = int(np.sum((ref == 1) | (ref == 2))) - int(np.sum((m == 1) | (m == 2)))
        assert off == 4 * ((dz + 4) + 9 * (dxy + 4))


def _params(**kw):
    return L_.make_params(**dict(dict(p=0.1, eta=3.0, alpha=1.5, iters=10, steps=10, p_logical=0.5), **kw))


def _plan(T, pr, cu_count=256):
    """validate_params() and plan_host() (csrc/plan_host.hpp): rc, message, the plan's kernel shape, lds_bytes, the persistent grid"""
    shape, msg, lds, grid = np.zeros(25, np.int32), C.create_string_buffer(600), C.c_uint64(), C.c_uint32()
    rc = T.qt_plan(C.byref(pr), cu_count, shape.ctypes.data, C.byref(lds), C.byref(grid), msg, len(msg))
    return rc, msg.value.decode(), shape, lds.value, grid.value


@pytest.mark.parametrize("code,L", SHAPES)
def test_plan_host_answers_every_block(T, code, L):
    """every rule, scan and ladder length: a plan, or a refusal with its code and a message"""
    plans = 0
    for noise, scan, Nc, conv in [(n, s, c, v) for n in range(3) for s in range(4) for c in (1, 2, 8, 16) for v in (0, 1)]:
        rc, msg, shape, lds, grid = _plan(T, _params(code=code, L=L, noise=noise, scan=scan, Nc=Nc, conv_mode=conv))
        assert rc in (0, -1, -4) and (rc == 0) == (msg == ""), (noise, scan, Nc, conv, rc, msg)
        if rc == 0:
            plans += 1
            assert 0 < lds <= 160 * 1024 and list(shape[:5]) == [code, noise, scan, L, Nc] and shape[6] == _nq(code, L)
            assert grid == 0 or conv
    assert plans >= 20


# the refusals of plan_host() that parameter blocks reach (validate_params() accepts each of these blocks), in the words they always had
@pytest.mark.parametrize("kw,text", [
    (dict(code=TORIC, L=33), "L=33: 2178 generators exceed the LDS table of 2048 (needed by scan=1 and by the xzzx / rotated codes)"),
    (dict(code=XZZX, L=23, noise=1), "biased / alpha noise packs the error counts in 10-bit fields: nq=529"),
    (dict(code=ROTATED, L=23, noise=2, scan=3, Nc=2), "biased / alpha noise packs the error counts in 10-bit fields: nq=529"),
    (dict(code=TORIC, L=32, Nc=16), "L=32 Nc=16 needs # B of LDS per workgroup (> 160 KiB)"),
    (dict(code=TORIC, L=32, Nc=16, scan=2), "scan = colour: L=32 Nc=16 needs # B of LDS per workgroup (> 160 KiB)"),
    (dict(code=XZZX, L=5, Nc=2, noise=1, scan=2, p=1e-100), "scan = colour: an acceptance ratio of rung 0 underflows"),
    (dict(code=TORIC, L=17, Nc=4, scan=3),
     "scan = wave: L=17 Nc=4 p=0.1 is outside what it is built for (depolarizing rule: a top rung that accepts every move, at most 16 packed state "
     "words per rung -- toric / planar L <= 11, xzzx / rotated L <= 16 --, fixed-length runs of up to 8 rungs 32 words -- toric L <= 16, xzzx / "
     "rotated L <= 22; alpha rule: xzzx / rotated L <= 11, 4 iters max|log2 ratio| <= 2000 --, # B of LDS)"),
])
def test_plan_refusals_keep_their_words(T, kw, text):
    rc, msg, _, _, _ = _plan(T, _params(**kw))
    rx = re.escape(text).replace(re.escape("#"), r"\d+")       # (#: a byte count; everything else to the letter)
    assert rc == -4 and re.fullmatch(rx, msg), msg


PLANS = [dict(code=TORIC, L=5, Nc=5), dict(code=XZZX, L=5, Nc=3, noise=1), dict(code=ROTATED, L=5, Nc=4, noise=2, scan=3, conv_mode=1),
         dict(code=XZZX, L=5, Nc=3, noise=2, scan=2), dict(code=PLANAR, L=4, Nc=8, scan=1)]


@pytest.mark.parametrize("kw", PLANS)
def test_plan_key_drops_what_no_plan_depends_on(T, kw):
    """blocks that differ in seed, first_syndrome or steps share a key and a host plan (tables, scalars, lds_bytes, shape, queue; the seed itself,
    which plan_host() copies into the launch arguments and the cached step path patches per call, set aside)"""
    a = _params(**kw)
    for other in (dict(seed=7), dict(first_syndrome=128), dict(steps=99), dict(seed=2 ** 40 + 3, first_syndrome=64, steps=1)):
        b = _params(**dict(kw, **other))
        assert T.qt_plan_key_equal(C.byref(a), C.byref(b)) == 1 and T.qt_plan_equal(C.byref(a), C.byref(b)) == 1, other


@pytest.mark.parametrize("field,base,other", [
    ("code", dict(code=TORIC, L=5), PLANAR), ("L", dict(L=5), 6), ("Nc", dict(L=5), 6), ("noise", dict(code=XZZX, L=5), 1), ("scan", dict(L=5), 1),
    ("conv_mode", dict(L=5), 1), ("iters", dict(L=5), 11), ("tops_burn", dict(L=5), 3), ("TOPS", dict(L=5), 11), ("SEQ", dict(L=5), 3),
    ("replicas", dict(L=5), 2), ("eps", dict(L=5), 0.2), ("p", dict(L=5), 0.11), ("eta", dict(code=XZZX, L=5, noise=1), 4.0),
    ("alpha", dict(code=XZZX, L=5, noise=2), 1.6), ("p_logical", dict(L=5), 0.4), ("flags", dict(L=5), 2), ("device", dict(L=5), 1)])
def test_plan_key_keeps_what_a_plan_depends_on(T, field, base, other):
    """each field of the key: two accepted blocks that differ in it have different keys -- and different host plans, but for the device, which only
    says where the tables go"""
    a, b = _params(Nc=5, **base), _params(**dict(dict(Nc=5, **base), **{field: other}))
    assert T.qt_plan_key_equal(C.byref(a), C.byref(a)) == 1 and T.qt_plan_key_equal(C.byref(a), C.byref(b)) == 0
    assert T.qt_plan_equal(C.byref(a), C.byref(b)) == (1 if field == "device" else 0)


@pytest.mark.parametrize("kw", [dict(code=TORIC, L=9, Nc=8), dict(code=XZZX, L=5, Nc=5, noise=2),
                                dict(code=TORIC, L=9, Nc=8, scan=3), dict(code=XZZX, L=5, Nc=5, noise=2, scan=3)])
def test_workspace_need_is_its_closed_form(T, kw):
    """2 bytes (alpha: 4) per ladder step and column; a column per ladder, rounded up to whole groups of 64 -- with the work queue, a column per lane
    of the persistent grid: the ladder family's grid, capped by the batch; scan = wave's as many workgroups as own a whole number of 64-ladder
    groups each"""
    steps = 37
    rc, msg, _, _, grid = _plan(T, _params(conv_mode=1, steps=steps, **kw))
    assert rc == 0 and grid > 0, msg
    up64 = lambda v: (v + 63) // 64 * 64
    for replicas, N, queue in [(r, n, q) for r in (1, 3) for n in (1, 64, 1000, 65536) for q in (0, 1)]:
        M = N * replicas
        cols = up64(M)
        if queue and kw.get("scan") == 3:
            g = max(1, min(grid, up64(M) // 64))
            chunk = up64(-(-M // g))
            cols = -(-M // chunk) * 64
        elif queue:
            cols = min(cols, grid * 64)
        pr = _params(conv_mode=1, steps=steps, replicas=replicas, **kw)
        assert T.qt_workspace_need(C.byref(pr), grid, N, queue) == (4 if kw.get("noise") == 2 else 2) * cols * steps, (replicas, N, queue)
        assert T.qt_workspace_need(C.byref(_params(steps=steps, replicas=replicas, **kw)), grid, N, queue) == 0       # fixed-length runs log nothing


def test_host_tables_under_asan_ubsan():
    if os.environ.get("QECMC_TABLES_LIB"):
        pytest.skip("already the sanitizer child")
    subprocess.check_call(["make", "-C", CSRC, "-s", "tables_asan"])
    libasan = subprocess.check_output(["g++", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(libasan):
        pytest.skip("libasan not installed")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1", LD_PRELOAD=libasan,
               QECMC_TABLES_LIB=os.path.join(CSRC, "build", "libqecmc_tables_asan.so"))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
