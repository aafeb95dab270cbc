"""Who walks the swap cascade of a scan = wave step (csrc/kernel_choice.hpp wave_cascade_once(), what a launch puts into LadderArgs::wu_once): the top
rung's wave once per workgroup, or every wave for itself.  Eligible are the shapes ladder_kernel's SSW variant is chosen for -- fixed length,
depolarizing rule, at most 16 state words, workgroups of up to 512 threads of which four fit a CU's 160 KiB of LDS --; among them the same-box A/B
decides (once per workgroup is 2.6 - 5.2 % faster at 5, 6 and 7 rungs, whatever the code and the width, and 0.5 - 3.8 % slower at 2, 3, 4
and 8 rungs -- config 2's ladder, 57.2 against 56.6 ms --, so config 2 keeps the replay).  QECMC_FLAG_NO_SSW (flags bit 8) asks for the replay everywhere.
Host code only: asked through the g++-built test API (csrc/tables_test_api.cpp), no GPU."""
import ctypes as C

import numpy as np
import pytest

from hostlib import PLANAR, ROTATED, TORIC, XZZX, ask, tables_lib
from hostlib import launch_shape as shape

NO_SSW = 8


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_wave_cascade_once.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def once(T, shapes):
    return ask(T.qt_wave_cascade_once, shapes)


def family(T, s):
    keys = np.zeros(11, dtype=np.int64)
    T.qt_choose_kernels(np.array(s, dtype=np.int32).ctypes.data, 1, keys.ctypes.data)
    return int(keys[0])


def test_config_2_replays_with_and_without_flag_8(T):
    """the headline shape: eight rungs, where the once-per-workgroup form measured slower than the replay, so the choice keeps the replay"""
    assert once(T, [shape(T, TORIC, 9, 8), shape(T, TORIC, 9, 8, tune=NO_SSW)]) == [0, 0]


def test_config_2s_lattice_walks_it_once_at_five_to_seven_rungs_and_flag_8_replays(T):
    assert once(T, [shape(T, TORIC, 9, Nc) for Nc in range(2, 9)]) == [0, 0, 0, 1, 1, 1, 0]
    assert once(T, [shape(T, TORIC, 9, Nc, tune=NO_SSW) for Nc in range(2, 9)]) == [0] * 7
    # ... whatever the other developer bits say, and for every iters (the switch is no part of the kernel key)
    assert once(T, [shape(T, TORIC, 9, 7, tune=2 | 4), shape(T, TORIC, 9, 7, tune=2 | 4 | NO_SSW), shape(T, TORIC, 9, 7, iters=7)]) == [1, 0, 1]


@pytest.mark.parametrize("code,L,Nc", [(TORIC, 3, 5), (TORIC, 5, 5), (TORIC, 7, 7), (TORIC, 11, 5), (XZZX, 9, 6), (ROTATED, 13, 7), (PLANAR, 5, 5)])
def test_fixed_length_shapes_of_which_four_fit_a_cu_walk_it_once(T, code, L, Nc):
    s = shape(T, code, L, Nc)
    assert family(T, s) == 2
    assert once(T, [s, shape(T, code, L, Nc, tune=NO_SSW)]) == [1, 0]


def test_criterion_alpha_and_32_word_shapes_replay(T):
    for s in (shape(T, TORIC, 9, 6, conv=1), shape(T, TORIC, 9, 6, conv=1, queue=1),          # the criterion / queue kernels
              shape(T, XZZX, 5, 5, noise=2), shape(T, ROTATED, 7, 6, noise=2, conv=1),        # the alpha rule
              shape(T, TORIC, 15, 6), shape(T, ROTATED, 21, 7), shape(T, TORIC, 12, 5)):      # 29, 28 and 18 words: the 32-word kernels
        assert family(T, s) == 2, s
        assert once(T, [s]) == [0], s


def test_fewer_than_four_workgroups_per_cu_replay(T):
    # toric L = 9 from nine rungs on: 1 024-thread workgroups of more than 40 KiB
    assert once(T, [shape(T, TORIC, 9, Nc) for Nc in range(9, 17)]) == [0] * 8
    # ... and seven rungs of the toric code's 16 words at L = 11: 28 KiB of states, more than 40 KiB with the records and tables
    assert once(T, [shape(T, TORIC, 11, 7)]) == [0]
    assert once(T, [shape(T, TORIC, 11, 5), shape(T, TORIC, 11, 6)]) == [1, 1]


def test_other_scans_and_refused_shapes_never_set_it(T):
    assert once(T, [shape(T, TORIC, 9, 6, scan=0), shape(T, TORIC, 9, 6, scan=2)]) == [0, 0]
    refused = shape(T, TORIC, 9, 6, lower_acc=1)                                              # a rung below the top at p = 0.75: no wave kernel
    assert family(T, refused) == 0 and once(T, [refused]) == [0]
