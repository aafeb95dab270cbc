"""The wave layout of the toric scan = "wave" kernels (csrc/tables.hpp wave_position, toric_wave_descriptors, wave_layout_rows; csrc/ladder_wu.hpp
wu_read_cell / wu_xor_cell): the two layers interleaved, qubit (layer, r, c) at field 2 (r L + c) + layer, so that the two qubits of a generator's
own cell are adjacent fields of one state word.  The tables are built here by g++ alone (no HIP, no GPU) and compared with the oracle: the position
function, the 32-byte descriptors interpreted the way the kernel reads them, the logical masks, what plan_host() hands a launch, and -- against a
recorded fixture -- that the flat descriptors of the other codes' kernels are what they were."""
import ctypes as C
import os

import numpy as np
import pytest

from hostlib import PLANAR, ROOT, ROTATED, TORIC, XZZX, tables_lib
from oracle import oracle as orc
from qecmc import _lib as L_

SIZES = [3, 4, 5, 9, 12, 16]


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_wave_position.restype = C.c_uint32; lib.qt_wave_position.argtypes = [C.c_int, C.c_int, C.c_uint32]
    lib.qt_plan_wave_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _positions(T, code, L, nq):
    return np.array([T.qt_wave_position(code, L, q) for q in range(nq)], np.int64)


def _pack(flat, pos, W):
    """fields at their wave-layout positions: field p in word p >> 4 at bit 2 (p & 15)"""
    words = [0] * W
    for q, f in enumerate(flat):
        words[pos[q] >> 4] |= int(f) << (2 * (pos[q] & 15))
    return words


def _unpack(words, pos):
    return np.array([(words[p >> 4] >> (2 * (p & 15))) & 3 for p in pos], np.uint8)


def _descriptors(T, L):
    G = 2 * L * L
    buf = np.zeros(8 * G, np.uint32)
    assert T.qt_toric_wave_descriptors(L, _ptr(buf), buf.size) == 8 * G
    return buf.reshape(G, 8)


def _generators(L, rng):
    G = 2 * L * L
    return range(G) if L <= 5 else rng.permutation(G)[:40]


@pytest.mark.parametrize("L", SIZES)
def test_position_is_a_bijection_that_interleaves_the_layers(T, L):
    nq = 2 * L * L
    pos = _positions(T, TORIC, L, nq)
    assert np.array_equal(np.sort(pos), np.arange(nq))
    q = np.arange(nq).reshape(2, L, L)
    for layer in range(2):
        assert np.array_equal(pos[q[layer]], 2 * (np.arange(L * L).reshape(L, L)) + layer)


@pytest.mark.parametrize("code,L", [(XZZX, 5), (ROTATED, 7), (PLANAR, 4)])
def test_position_is_the_identity_for_the_other_codes(T, code, L):
    nq = 2 * L * L if code == PLANAR else L * L
    assert np.array_equal(_positions(T, code, L, nq), np.arange(nq))


@pytest.mark.parametrize("L", SIZES)
def test_own_cell_pair_shares_a_word(T, L):
    nq = 2 * L * L; W = (nq + 15) // 16
    pos = _positions(T, TORIC, L, nq)
    d = _descriptors(T, L)
    for g in _generators(L, np.random.default_rng(L)):
        e = [int(x) for x in d[g]]
        r, c = (int(g) % (L * L)) // L, int(g) % L
        w, s0, s1 = e[0] & 0xFF, (e[0] >> 8) & 0xFF, (e[0] >> 16) & 0xFF
        assert e[0] >> 24 == 0 and w < W and s1 == s0 + 2 and s0 % 4 == 0 and s1 < 32
        # ... and it is the generator's own cell: (0, r, c) at the lower shift, (1, r, c) above it
        assert (pos[r * L + c], pos[L * L + r * L + c]) == (16 * w + s0 // 2, 16 * w + s1 // 2)
        P = 1 if g < L * L else 3
        assert e[3] == (5 * P) << s0 and e[7] == 0
        for i in (1, 2):
            assert e[i] >> 13 == 0 and (e[i] & 0xFF) < W and e[3 + i] == P << ((e[i] >> 8) & 31)


@pytest.mark.parametrize("L", SIZES)
def test_descriptors_read_the_kernels_way_are_the_oracles_stabilizer(T, L):
    """three word reads for four fields (v_lshrrev_b32_sdwa: a byte, junk above the field), the byte table behind v_perm_b32, v_sad_u8's byte sum, three XORs --
    on random states, against toric_apply_stabilizer: the new configuration and the change of the error count"""
    nq = 2 * L * L; W = (nq + 15) // 16
    pos = _positions(T, TORIC, L, nq)
    d = _descriptors(T, L)
    rng = np.random.default_rng(L * 5)
    for g in _generators(L, rng):
        m = rng.integers(0, 4, size=(2, L, L)).astype(np.uint8)
        words = _pack(m.ravel(), pos, W)
        e = [int(x) for x in d[g]]
        reads = [(e[0] & 0xFF, (e[0] >> 8) & 0xFF), (e[0] & 0xFF, (e[0] >> 16) & 0xFF), (e[1] & 0xFF, (e[1] >> 8) & 0xFF), (e[2] & 0xFF, (e[2] >> 8) & 0xFF)]
        sel = 0
        for i, (w, sh) in enumerate(reads):
            sel |= ((words[w] >> (sh & 31)) & 0xFF) << (8 * i)
        sel &= 0x03030303
        tab = e[6].to_bytes(4, "little")
        dE4 = sum(tab[(sel >> (8 * i)) & 0xFF] for i in range(4))
        for w, x in ((e[0] & 0xFF, e[3]), (e[1] & 0xFF, e[4]), (e[2] & 0xFF, e[5])):      # read-modify-writes in order: sites may share a word
            words[w] ^= x
        ref, dE = orc.toric_apply_stabilizer(m, (int(g) % (L * L)) // L, int(g) % L, 1 if g < L * L else 3)
        assert np.array_equal(_unpack(words, pos).reshape(m.shape), ref), g
        assert dE4 == 4 * (dE + 4), g


@pytest.mark.parametrize("L", SIZES)
def test_wave_layout_logical_masks_are_the_flat_ones_moved(T, L):
    nq = 2 * L * L; W = (nq + 15) // 16
    pos = _positions(T, TORIC, L, nq)
    flat, wave = np.zeros(4 * (L + 1) * W, np.uint32), np.zeros(4 * (L + 1) * W, np.uint32)
    assert T.qt_logical_masks(TORIC, L, W, _ptr(flat), flat.size) == flat.size
    assert T.qt_wave_logical_masks(TORIC, L, W, _ptr(wave), wave.size) == wave.size
    ident = np.arange(nq)
    for row_f, row_w in zip(flat.reshape(-1, W), wave.reshape(-1, W)):
        fields = _unpack([int(x) for x in row_f], ident)
        assert [int(x) for x in row_w] == _pack(fields, pos, W)
    assert flat.any() and not np.array_equal(flat, wave)


def _plan_tables(T, **kw):
    pr = L_.make_params(**dict(dict(p=0.1, eta=3.0, alpha=1.5, iters=10, steps=10, p_logical=0.5), **kw))
    desc, lmask, nd, nl = np.zeros(16 * 1024, np.uint32), np.zeros(4 * 32 * 32, np.uint32), C.c_int(), C.c_int()
    assert T.qt_plan_wave_tables(C.byref(pr), desc.ctypes.data, desc.size, C.byref(nd), lmask.ctypes.data, lmask.size, C.byref(nl)) == 0
    return desc[:nd.value].copy(), lmask[:nl.value].copy()


@pytest.mark.parametrize("L,Nc", [(3, 2), (5, 5), (9, 8), (12, 4)])
def test_a_toric_wave_plan_carries_the_wave_layout_and_no_other_plan_does(T, L, Nc):
    nq = 2 * L * L; W = (nq + 15) // 16
    flat, wave = np.zeros(4 * (L + 1) * W, np.uint32), np.zeros(4 * (L + 1) * W, np.uint32)
    T.qt_logical_masks(TORIC, L, W, _ptr(flat), flat.size)
    T.qt_wave_logical_masks(TORIC, L, W, _ptr(wave), wave.size)
    desc, lmask = _plan_tables(T, code=TORIC, L=L, Nc=Nc, scan=L_.SCAN_WAVE)
    assert np.array_equal(desc.reshape(-1, 8), _descriptors(T, L)) and np.array_equal(lmask, wave)
    for scan in (L_.SCAN_RANDOM, L_.SCAN_SWEEP, L_.SCAN_COLOUR):
        desc, lmask = _plan_tables(T, code=TORIC, L=L, Nc=Nc, scan=scan)
        assert desc.size == 0 and np.array_equal(lmask, flat)


@pytest.mark.parametrize("code,L", [(XZZX, 5), (ROTATED, 7), (PLANAR, 5)])
def test_the_other_codes_wave_plans_keep_the_flat_tables(T, code, L):
    nq = 2 * L * L if code == PLANAR else L * L
    W = (nq + 15) // 16
    flat, d16 = np.zeros(4 * (L + 1) * W, np.uint32), np.zeros(16 * 1024, np.uint32)
    T.qt_logical_masks(code, L, W, _ptr(flat), flat.size)
    n = T.qt_wave_descriptors(code, L, _ptr(d16), d16.size)
    desc, lmask = _plan_tables(T, code=code, L=L, Nc=4, scan=L_.SCAN_WAVE)
    assert n > 0 and np.array_equal(desc, d16[:n]) and np.array_equal(lmask, flat)


def test_flat_wave_descriptors_are_what_they_were(T):
    """qt_wave_descriptors for toric L = 5 as recorded before the wave layout existed (tests/golden/wave_descriptors_toric_L5.npz)"""
    want = np.load(os.path.join(ROOT, "tests", "golden", "wave_descriptors_toric_L5.npz"))["descriptors"]
    buf = np.zeros(want.size, np.uint32)
    assert T.qt_wave_descriptors(TORIC, 5, _ptr(buf), buf.size) == want.size
    assert np.array_equal(buf.reshape(want.shape), want)
