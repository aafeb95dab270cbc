"""What a scan = wave launch puts into LadderArgs::wu_once (csrc/kernel_choice.hpp wave_cascade_walk()): wave_cascade_once() -- the rule measured on the
plain once-per-workgroup form of the swap cascade, pinned by tests/test_wave_cascade_choice.py -- and the ladder length the form serves since the waves
below the top draw the next step's acceptance block in its wait (csrc/ladder_wu.hpp, the kernels with the unrolled loop of iters = 10): eight rungs,
config 2's ladder, as the same-box A/B of the two forms decided (profiles/r13_wave_walk_ab.json).  At eight rungs the new rule asks what
the old one asks: fixed length, depolarizing rule, at most 16 state words, 512-thread workgroups of which four fit a CU's 160 KiB of LDS, never a
statistics launch, and QECMC_FLAG_NO_SSW (flags bit 8) forces the replay.  Host code only: the g++-built test API (csrc/tables_test_api.cpp), no GPU."""
import ctypes as C

import pytest

from hostlib import KERNEL_SHAPE_FIELDS as FIELDS
from hostlib import PLANAR, ROTATED, TORIC, XZZX, tables_lib
from hostlib import ask as _ask
from hostlib import launch_shape as shape

NO_SSW = 8
WALK_AT_EIGHT_RUNGS = 1      # the A/B's answer


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_wave_cascade_once.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.qt_wave_cascade_walk.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def once(T, shapes):
    return _ask(T.qt_wave_cascade_once, shapes)


def walk(T, shapes):
    return _ask(T.qt_wave_cascade_walk, shapes)


def every_shape_of_the_cascade_choice_file(T):
    """the shapes tests/test_wave_cascade_choice.py asks wave_cascade_once() about"""
    out = [shape(T, TORIC, 9, Nc, tune=t) for Nc in range(2, 17) for t in (0, NO_SSW)]
    out += [shape(T, TORIC, 9, 7, tune=2 | 4), shape(T, TORIC, 9, 7, tune=2 | 4 | NO_SSW), shape(T, TORIC, 9, 7, iters=7)]
    for code, L, Nc in [(TORIC, 3, 5), (TORIC, 5, 5), (TORIC, 7, 7), (TORIC, 11, 5), (XZZX, 9, 6), (ROTATED, 13, 7), (PLANAR, 5, 5)]:
        out += [shape(T, code, L, Nc), shape(T, code, L, Nc, tune=NO_SSW)]
    out += [shape(T, TORIC, 9, 6, conv=1), shape(T, TORIC, 9, 6, conv=1, queue=1), shape(T, XZZX, 5, 5, noise=2), shape(T, ROTATED, 7, 6, noise=2, conv=1),
            shape(T, TORIC, 15, 6), shape(T, ROTATED, 21, 7), shape(T, TORIC, 12, 5), shape(T, TORIC, 11, 7), shape(T, TORIC, 11, 5), shape(T, TORIC, 11, 6),
            shape(T, TORIC, 9, 6, scan=0), shape(T, TORIC, 9, 6, scan=2), shape(T, TORIC, 9, 6, lower_acc=1)]
    return out


def test_the_walk_equals_the_once_rule_everywhere_but_at_eight_rungs(T):
    shapes = [s for s in every_shape_of_the_cascade_choice_file(T) if s[FIELDS.index("Nc")] != 8]
    assert len(shapes) > 50
    assert walk(T, shapes) == once(T, shapes)
    assert sum(walk(T, shapes)) >= 10                                                        # (the comparison is not one of zeros alone)


def test_wave_cascade_once_answers_as_before(T):
    assert once(T, [shape(T, TORIC, 9, Nc) for Nc in range(2, 9)]) == [0, 0, 0, 1, 1, 1, 0]
    assert once(T, [shape(T, TORIC, 9, 8), shape(T, TORIC, 9, 8, tune=NO_SSW)]) == [0, 0]
    assert once(T, [shape(T, code, L, 8) for code, L in [(TORIC, 3), (TORIC, 7), (XZZX, 9), (ROTATED, 13), (PLANAR, 5)]]) == [0] * 5


def test_eight_rungs_as_the_ab_decided(T):
    """config 2's ladder, and the other eligible shapes of eight rungs: every code, 4 / 8 / 12 / 16-word kernels"""
    assert walk(T, [shape(T, TORIC, 9, 8)]) == [WALK_AT_EIGHT_RUNGS]
    eight = [shape(T, TORIC, 3, 8), shape(T, TORIC, 5, 8), shape(T, TORIC, 7, 8), shape(T, XZZX, 9, 8), shape(T, ROTATED, 13, 8), shape(T, PLANAR, 5, 8),
             shape(T, XZZX, 13, 8)]
    assert walk(T, eight) == [WALK_AT_EIGHT_RUNGS] * len(eight)
    # the general loop keeps its draw at the top of the step: the plain once form, which lost at eight rungs
    assert walk(T, [shape(T, TORIC, 9, 8, iters=7), shape(T, TORIC, 9, 8, iters=1)]) == [0, 0]


def test_flag_8_forces_the_replay(T):
    assert walk(T, [shape(T, TORIC, 9, Nc, tune=NO_SSW) for Nc in range(2, 17)]) == [0] * 15
    assert walk(T, [shape(T, TORIC, 9, 8, tune=2 | 4 | NO_SSW), shape(T, XZZX, 9, 8, tune=NO_SSW)]) == [0, 0]
    assert walk(T, [shape(T, TORIC, 9, 8, tune=2 | 4)]) == [WALK_AT_EIGHT_RUNGS]             # (the other developer bits do not enter)


def test_statistics_launches_never_walk(T):
    assert walk(T, [shape(T, TORIC, 9, Nc, stats=1) for Nc in range(2, 9)]) == [0] * 7


def test_criterion_alpha_and_32_word_shapes_replay_at_eight_rungs_too(T):
    for s in (shape(T, TORIC, 9, 8, conv=1), shape(T, TORIC, 9, 8, conv=1, queue=1),          # the criterion / queue kernels
              shape(T, XZZX, 5, 8, noise=2), shape(T, ROTATED, 7, 8, noise=2, conv=1),        # the alpha rule
              shape(T, TORIC, 15, 8), shape(T, ROTATED, 21, 8), shape(T, TORIC, 12, 8)):      # 29, 28 and 18 words: the 32-word kernels
        assert walk(T, [s]) == [0], s


def test_fewer_than_four_workgroups_per_cu_replay(T):
    # eight rungs of the toric code's 16 words at L = 11: 32 KiB of states; nine rungs and more: 1 024-thread workgroups
    assert walk(T, [shape(T, TORIC, 11, 8), shape(T, TORIC, 11, 7)]) == [0, 0]
    assert walk(T, [shape(T, TORIC, 9, Nc) for Nc in range(9, 17)]) == [0] * 8
    assert walk(T, [shape(T, TORIC, 5, Nc) for Nc in range(9, 17)]) == [0] * 8


def test_other_scans_and_refused_shapes_never_walk(T):
    assert walk(T, [shape(T, TORIC, 9, 8, scan=0), shape(T, TORIC, 9, 8, scan=2)]) == [0, 0]
    refused = shape(T, TORIC, 9, 8, lower_acc=1)
    assert walk(T, [refused]) == [0]
