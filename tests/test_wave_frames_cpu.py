"""The top rung's frames of the scan = "wave" kernels (csrc/wu_frames.hpp): the top rung accepts every move and a wavefront shares its picks, so the ten
moves of a ladder step are one XOR mask of the state's words plus a class change, built once per pick window.  The builder is a host-callable inline
function; here it runs through the plain tables library (g++ alone, no HIP, no GPU) on given pick words, and a window's rows must equal applying the same
operators one after another to a byte state with the oracle's stabilizer and logical routines -- the configuration and the equivalence class."""
import ctypes as C

import numpy as np
import pytest

from hostlib import PLANAR, ROTATED, TORIC, XZZX, tables_lib
from oracle import oracle as orc
from qecmc import _lib as L_

P_LOGICAL = [0.0, 0.25, 0.5, 1.0]
CASES = [(TORIC, 3), (TORIC, 4), (TORIC, 9), (TORIC, 11), (XZZX, 9), (XZZX, 5), (ROTATED, 7), (PLANAR, 5)]


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_wave_position.restype = C.c_uint32; lib.qt_wave_position.argtypes = [C.c_int, C.c_int, C.c_uint32]
    lib.qt_wave_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def _shape(code, L):
    return (2, L, L) if code in (TORIC, PLANAR) else (L, L)


def _frames(T, code, L, p_logical, picks, iters=10):
    pr = L_.make_params(code=code, L=L, Nc=4, p=0.1, p_logical=p_logical, iters=iters, steps=10, scan=L_.SCAN_WAVE)
    buf = np.zeros(128 * 17, np.uint32)
    WV = T.qt_wave_frames(C.byref(pr), picks.ctypes.data, buf.ctypes.data, buf.size)
    assert WV in (4, 8, 12, 16)
    return buf[:(128 // iters) * (WV + 1)].reshape(128 // iters, WV + 1), WV


def _apply_mask(T, code, L, m, words):
    """state ^= the mask, field p of the packed words being qubit q with p = wave_position(q)"""
    flat = m.ravel().copy()
    for q in range(flat.size):
        p = T.qt_wave_position(code, L, q)
        flat[q] ^= (int(words[p >> 4]) >> (2 * (p & 15))) & 3
    return flat.reshape(m.shape)


def _oracle_move(code, L, m, A, B, thr16, G):
    """one move of the top rung (chain_update_wave of the oracle, by its exported stencils): logical iff A[31:16] < thr16"""
    A, B = int(A), int(B)
    if thr16 != 0 and (A >> 16) < thr16:
        if code == TORIC:
            ops = ((A >> 14) & 3, (A >> 12) & 3)
            for layer, op in enumerate(ops):
                xpos = zpos = 0
                if op in (1, 2):
                    xpos = ((A & 0xFFF) * L) >> 12 if layer == 0 else (((B >> 10) & 0x7FF) * L) >> 11
                if op in (3, 2):
                    zpos = ((B >> 21) * L) >> 11 if layer == 0 else ((B & 0x3FF) * L) >> 10
                m, _ = orc.toric_apply_logical(m, op, layer, xpos, zpos)
            return m
        op = (A >> 14) & 3
        xpos = ((A & 0x3FFF) * L) >> 14 if op in (1, 2) else 0
        zpos = ((B >> 16) * L) >> 16 if op in (3, 2) else 0
        return orc.surf_apply_logical(code, m, op, xpos, zpos)[0]
    g = (B * G) >> 32
    if code == TORIC:
        op = 1 if g < L * L else 3
        g %= L * L
        return orc.toric_apply_stabilizer(m, g // L, g % L, op)[0]
    r, c, op = orc.surf_gen_rco(code, L, g)
    return orc.surf_apply_stabilizer(code, m, r, c, op)[0]


def _cls(code, m):
    return orc.toric_eq_class(m) if code == TORIC else orc.surf_eq_class(code, m)


def _kernel_class(code, cls):
    """the class as the wave kernels keep it (xzzx: the internal value v with class = v ^ (v >> 1))"""
    return {0: 0, 1: 1, 2: 3, 3: 2}[cls] if code == XZZX else cls


@pytest.mark.parametrize("p_logical", P_LOGICAL)
@pytest.mark.parametrize("code,L", CASES)
def test_a_windows_frames_are_the_moves_applied_one_by_one(T, code, L, p_logical):
    rng = np.random.default_rng(1000 * code + 10 * L + int(4 * p_logical))
    picks = rng.integers(0, 1 << 32, size=(64, 4), dtype=np.uint64).astype(np.uint32)
    # (selector words on both sides of the threshold and at it, operator fields of every value, positions at the ends of their range)
    thr16 = int(np.ceil(p_logical * 65536))
    picks[0, 0] = (max(thr16 - 1, 0) << 16) | 0xBFFF; picks[0, 1] = 0xFFFFFFFF
    picks[0, 2] = (min(thr16, 0xFFFF) << 16) | 0x4000; picks[0, 3] = 0
    frames, WV = _frames(T, code, L, p_logical, picks)
    G = 2 * L * L if code == TORIC else orc.surf_ngen(code, L)
    logical = stabilizer = 0
    for s in range(12):
        m0 = rng.integers(0, 4, size=_shape(code, L)).astype(np.uint8)
        if code == PLANAR:
            m0[1, -1, :] = 0; m0[1, :, -1] = 0
        m = m0
        for j in range(10):
            P = 10 * s + j
            A, B = picks[P >> 1, 2 * (P & 1)], picks[P >> 1, 2 * (P & 1) + 1]
            is_log = thr16 != 0 and (int(A) >> 16) < thr16
            logical += is_log; stabilizer += not is_log
            m = _oracle_move(code, L, m, A, B, thr16, G)
        got = _apply_mask(T, code, L, m0, frames[s, :WV])
        assert np.array_equal(got, m), (code, L, p_logical, s)
        assert _kernel_class(code, _cls(code, m0)) ^ int(frames[s, WV]) == _kernel_class(code, _cls(code, m)), (code, L, p_logical, s)
    assert (logical > 0) == (p_logical > 0) and (stabilizer > 0) == (p_logical < 1)


def test_proposals_beyond_the_windows_last_step_are_left_out(T):
    """128 = 12 x 10 + 8: the picks of lanes 60 .. 63 belong to no step and must not reach a row"""
    rng = np.random.default_rng(5)
    picks = rng.integers(0, 1 << 32, size=(64, 4), dtype=np.uint64).astype(np.uint32)
    a, _ = _frames(T, TORIC, 9, 0.5, picks)
    picks[60:] = rng.integers(0, 1 << 32, size=(4, 4), dtype=np.uint64).astype(np.uint32)
    b, _ = _frames(T, TORIC, 9, 0.5, picks)
    assert np.array_equal(a, b) and a.any()


def test_the_frame_buffer_is_part_of_the_plans_lds(T):
    """qecmc_plan_info's LDS bytes follow wu_lds(): the lean kernels with the unrolled loop (fixed length, iters = 10, up to 16 words) carry
    12 rows of WV + 1 words -- 624 B at the headline shape, four workgroups of which still share a CU's 160 KiB --, no other kernel does"""
    def lds(**kw):
        pr = L_.make_params(**dict(dict(code=TORIC, L=9, Nc=8, p=0.1, p_logical=0.5, iters=10, steps=10, scan=L_.SCAN_WAVE), **kw))
        T.qt_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        shape = np.zeros(64, np.int32); n = C.c_uint64(); grid = C.c_uint32(); msg = C.create_string_buffer(256)
        assert T.qt_plan(C.byref(pr), 256, shape.ctypes.data, C.byref(n), C.byref(grid), msg, 256) == 0, msg.value
        return n.value
    assert lds() - lds(iters=9) == 4 * 12 * 13 == 624 and 4 * lds() <= 160 * 1024
    assert lds(L=3, Nc=2) - lds(L=3, Nc=2, iters=7) == 4 * 12 * 5
    assert lds(L=11) - lds(L=11, iters=3) == 4 * 12 * 17
    assert lds(L=12) == lds(L=12, iters=9)                                             # 32 words: the general tail, no frames
    conv = dict(conv_mode=L_.CONV_ERROR_BASED, TOPS=4, SEQ=2, eps=0.3)
    assert lds(**conv) == lds(iters=9, **conv)                                         # the criterion kernels
