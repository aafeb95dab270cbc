"""Which form of the once-per-workgroup swap cascade a scan = wave launch runs (csrc/kernel_choice.hpp wave_cascade_mode(), what ladder_rs.hip puts into
LadderArgs::wu_once): 0 the replay, 1 the walk with the top rung's wave turning both blocks of swap uniforms into bounds in front of the step's first
barrier, 2 the walk with the bounds spread over the waves below the top, a pair each (csrc/ladder_wu.hpp, the lean step tail).  The mode is 0 exactly where
wave_cascade_walk() says no; 2 only for the kernels whose top wave draws both blocks (fixed length, depolarizing rule, at most 16 words, iters = 10, at
most 8 rungs) at the ladder lengths where the same-box A/B had the spread form ahead (kSpreadRungs; DESIGN.md 4.1g, profiles/r15_wave_spread_ab.json);
1 otherwise.  QECMC_FLAG_NO_SPREAD (flags bit 16) turns a 2 into a 1, QECMC_FLAG_NO_SSW (bit 8) gives 0.  Host code only: the g++-built test API
(csrc/tables_test_api.cpp), no GPU."""
import ctypes as C
import itertools

import pytest

from hostlib import KERNEL_SHAPE_FIELDS as FIELDS
from hostlib import PLANAR, ROTATED, TORIC, XZZX, tables_lib
from hostlib import ask as _ask
from hostlib import launch_shape as shape

NO_SSW, NO_SPREAD = 8, 16
SPREAD_RUNGS = (8,)      # the A/B's answer: the ladder lengths at which the spread form cleared the bar (profiles/r15_wave_spread_ab.json)
# a lattice size per state width (4, 8, 12, 16 words per rung) of every code
WIDTHS = {TORIC: (3, 7, 9, 11), XZZX: (5, 9, 13, 15), ROTATED: (5, 9, 13, 15), PLANAR: (3, 7, 9, 11)}


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_wave_cascade_walk.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.qt_wave_cascade_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def walk(T, shapes):
    return _ask(T.qt_wave_cascade_walk, shapes)


def mode(T, shapes):
    return _ask(T.qt_wave_cascade_mode, shapes)


def _f(s, name):
    return s[FIELDS.index(name)]


def top_draws(s):
    """the kernel of an eligible shape is one whose top wave draws both blocks: the unrolled loop of iters = 10 on at most 8 rungs (ladder_wu.hpp TOPDRAWS;
    fixed length, the depolarizing rule and at most 16 words are what wave_cascade_walk() already asks)"""
    return _f(s, "iters") == 10 and _f(s, "Nc") <= 8


@pytest.fixture(scope="module")
def grid(T):
    """all codes, the four state widths, 2 .. 16 rungs, iters 10 and 7, fixed length and criterion, plain and statistics launches, tune 0 / 8 / 16"""
    out = []
    for code in (TORIC, XZZX, ROTATED, PLANAR):
        for L, Nc, iters, conv, stats, tune in itertools.product(WIDTHS[code], range(2, 17), (10, 7), (0, 1), (0, 1), (0, NO_SSW, NO_SPREAD)):
            out.append(shape(T, code, L, Nc, iters=iters, conv=conv, stats=stats, tune=tune))
    return out


def test_the_grid_covers_the_four_widths_of_every_code(grid):
    assert {(_f(s, "code"), _f(s, "W") if _f(s, "W") % 4 == 0 else _f(s, "W") + 4 - _f(s, "W") % 4) for s in grid} >= {
        (c, w) for c in (TORIC, XZZX, ROTATED, PLANAR) for w in (4, 8, 12, 16)}


def test_mode_is_zero_exactly_where_the_launch_does_not_walk(T, grid):
    w, m = walk(T, grid), mode(T, grid)
    assert all((mi == 0) == (wi == 0) for wi, mi in zip(w, m))
    assert set(m) <= {0, 1, 2} and sum(w) > 100


def test_mode_two_only_on_the_top_draw_kernels_at_the_measured_lengths(T, grid):
    w, m = walk(T, grid), mode(T, grid)
    for s, wi, mi in zip(grid, w, m):
        want = 0 if not wi else 2 if top_draws(s) and _f(s, "Nc") in SPREAD_RUNGS and not _f(s, "tune") & NO_SPREAD else 1
        assert mi == want, (dict(zip(FIELDS, s)), wi, mi)
    # (the general loop walks at 5 - 7 rungs and is no top-draw kernel: mode 1 is not an empty set)
    assert 1 in m


def test_flag_16_turns_two_into_one_and_nothing_else(T, grid):
    plain = [s for s in grid if _f(s, "tune") == 0]
    flagged = [s[:-1] + [NO_SPREAD] for s in plain]
    assert FIELDS[-1] == "tune"
    for a, b in zip(mode(T, plain), mode(T, flagged)):
        assert b == (1 if a == 2 else a)
    assert walk(T, plain) == walk(T, flagged)


def test_flag_8_gives_zero(T, grid):
    assert set(mode(T, [s for s in grid if _f(s, "tune") == NO_SSW])) == {0}
    assert mode(T, [shape(T, TORIC, 9, 8, tune=NO_SSW | NO_SPREAD), shape(T, TORIC, 9, 6, tune=NO_SSW | NO_SPREAD)]) == [0, 0]


def test_config_2_as_the_ab_decided(T):
    """toric L = 9, 8 rungs, iters = 10: the headline launch"""
    assert mode(T, [shape(T, TORIC, 9, 8)]) == [2 if 8 in SPREAD_RUNGS else 1]
    assert mode(T, [shape(T, TORIC, 9, 8, tune=NO_SPREAD)]) == [1]
    assert mode(T, [shape(T, TORIC, 9, Nc) for Nc in range(2, 10)]) == [0, 0, 0] + [2 if Nc in SPREAD_RUNGS else 1 for Nc in (5, 6, 7, 8)] + [0]


def test_statistics_criterion_alpha_and_wide_shapes_stay_at_zero(T):
    for s in (shape(T, TORIC, 9, 8, stats=1), shape(T, TORIC, 9, 8, conv=1), shape(T, TORIC, 9, 8, conv=1, queue=1), shape(T, XZZX, 5, 8, noise=2),
              shape(T, TORIC, 15, 8), shape(T, TORIC, 11, 8), shape(T, TORIC, 9, 8, scan=0), shape(T, TORIC, 9, 8, lower_acc=1)):
        assert mode(T, [s]) == [0], s
