"""The statistics kernels of scan = wave and scan = colour (qecmc_plan_set_stats; csrc/kernel_choice.hpp choose_wave / choose_colour, csrc/ladder_wu.hpp
STATS, csrc/ladder_colour.hpp), on the CPU: what the chooser answers to stats = 1 on scans 2 and 3 -- which tests/test_kernel_choice.py never presents
there --, that the answer never touches a stats = 0 shape, that every statistics key names a kernel in the build and every built statistics kernel is
chosen, and the register / scratch budget of those kernels (a label outside the frozen allow-list of tests/test_kernel_resources.py may use no scratch).
Host code only: asked through the g++-built test API (csrc/tables_test_api.cpp), as tests/test_kernel_choice.py does."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest

from hostlib import ROOT, resource_rows, tables_lib


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# the sweep's building blocks (every code, rule, scan and L the library makes plans of; the temperature ladders a plan presents) are the frozen ones
KC = _load("test_kernel_choice", os.path.join(ROOT, "tests", "test_kernel_choice.py"))
FIELDS, CODES = KC.FIELDS, KC.CODES
KEY_STATS = 1                       # KernelKey::flags of a statistics kernel (kernel_choice.hpp kKeyStats); 0 for every other wave / colour kernel
# the refusals that name the case (qecmc_plan_set_stats hands them to the caller as QECMC_ERR_UNSUPPORTED)
WAVE_CRITERION = "scan = wave: swap statistics are collected in fixed-length runs only, not with the criterion"
WAVE_WIDE = "scan = wave: no swap statistics above 16 state words per rung (the 32-word kernels' staging spills)"
COLOUR_CRITERION = "scan = colour: swap statistics are collected in fixed-length runs only, not with the criterion"
ONE_RUNG = "swap statistics need Nc >= 2"


@pytest.fixture(scope="module")
def T():
    lib = tables_lib()
    lib.qt_wave_cascade_once.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def keys_of(T, shapes):
    shapes = np.ascontiguousarray(shapes, dtype=np.int32)
    keys = np.zeros((len(shapes), 11), dtype=np.int64)
    T.qt_choose_kernels(shapes.ctypes.data, len(shapes), keys.ctypes.data)
    return keys


def stats_label(key):
    """a statistics kernel as tools/kernel_resources.py labels it"""
    family, maxt, minw, code, flags, wv, conv, it, alpha, rule, _ = (int(x) for x in key)
    assert flags == KEY_STATS and (maxt, minw, conv, it) == (1024, 4, 0, 0), key
    if family == 2:
        return "wave-stats<1024,4,%s: %d words%s>" % (CODES[code], wv, ", alpha" if alpha else "")
    assert family == 3 and (wv, alpha) == (0, 0), key
    return "colour-stats<1024,4,%s: rule %d>" % (CODES[code], rule)


def why(key):
    return C.string_at(int(key[10])).decode()


@pytest.fixture(scope="module")
def sweep(T):
    """stats = 0 and stats = 1 of every fixed-length / criterion launch of scans 2 and 3: code, L, rule, Nc = 1 .. 16, both temperature ladders of the rule,
    logical moves on and off, iters 10 / 7 / 200.  Returns {statistics label: shapes}, {refusal of a stats = 1 shape whose stats = 0 twin has a kernel: shapes}."""
    chosen, refused, n = {}, {}, 0
    for base in KC.blocks(T):
        noise, scan = base["noise"], base["scan"]
        if scan not in (2, 3):
            continue
        rows = []
        for Nc in range(1, 17):
            for (top, lower, sfo, f32), conv, logical, iters in itertools.product(KC.ladders(noise, scan, Nc), (0, 1), (0, 1), (10, 7, 200)):
                s = dict(base, Nc=Nc, top_acc=top, lower_acc=lower, swap_fast_ok=sfo, f32ok=f32, conv=conv, queue=0, uset=0, xyz=0, stats=0, resume=0, neff=0,
                         logical=logical, iters=iters, tune=0)
                rows.append([s[f] for f in FIELDS])
        plain = np.array(rows, dtype=np.int32)
        withs = plain.copy()
        withs[:, FIELDS.index("stats")] = 1
        kp, ks = keys_of(T, plain), keys_of(T, withs)
        n += len(rows)
        for s, a, b in zip(plain, kp, ks):
            sh = dict(zip(FIELDS, (int(x) for x in s)))
            # stats = 0: exactly the fast kernels' keys, whose flags are 0 in both families
            assert a[4] == 0, (sh, a)
            if a[0] == 0:
                # no kernel without statistics: none with them, for the same reason
                assert b[0] == 0 and why(b) == why(a), (sh, why(a), why(b))
                continue
            assert a[0] == (2 if scan == 3 else 3)
            if b[0] == 0:
                r = why(b)
                refused[r] = refused.get(r, 0) + 1
                # each named refusal exactly where the issue puts it
                if scan == 3:
                    assert r == (WAVE_CRITERION if sh["conv"] else WAVE_WIDE), (sh, r)
                    assert sh["conv"] or sh["W"] > 16, (sh, r)
                else:
                    assert r == (COLOUR_CRITERION if sh["conv"] else ONE_RUNG), (sh, r)
                    assert sh["conv"] or sh["Nc"] < 2, (sh, r)
                continue
            # a statistics key: the fast kernel's family and code, a field operator== compares apart, fixed length, the general proposal loop
            assert b[0] == a[0] and b[3] == a[3] and b[4] == KEY_STATS and not sh["conv"] and sh["Nc"] >= 2, (sh, a, b)
            assert (b[5], b[8], b[9]) == (a[5], a[8], a[9]) and b[5] <= 16, (sh, a, b)        # the state width, the rule
            lab = stats_label(b)
            chosen[lab] = chosen.get(lab, 0) + 1
    return dict(chosen=chosen, refused=refused, shapes=n)


def test_stats_shapes_get_a_statistics_key_or_a_named_refusal(sweep):
    assert sweep["shapes"] > 50000
    assert set(sweep["refused"]) == {WAVE_CRITERION, WAVE_WIDE, COLOUR_CRITERION, ONE_RUNG}
    # all four codes at all four widths under the depolarizing rule, the alpha rule on xzzx / rotated at 4 and 8 words; every code and rule of scan = colour
    want = {"wave-stats<1024,4,%s: %d words>" % (c, w) for c in CODES for w in (4, 8, 12, 16)}
    want |= {"wave-stats<1024,4,%s: %d words, alpha>" % (c, w) for c in ("xzzx", "rotated") for w in (4, 8)}
    want |= {"colour-stats<1024,4,%s: rule 0>" % c for c in CODES} | {"colour-stats<1024,4,%s: rule %d>" % (c, r) for c in ("xzzx", "rotated") for r in (1, 2)}
    assert set(sweep["chosen"]) == want


@pytest.fixture(scope="module")
def built():
    """label -> row of every statistics kernel in csrc/build/*.res"""
    rows = resource_rows()
    assert len(rows) > 100
    return {r["label"]: r for r in rows if r["label"].startswith(("wave-stats<", "colour-stats<"))}, rows


def test_every_statistics_key_is_built_and_every_built_statistics_kernel_is_chosen(sweep, built):
    stats_rows, _ = built
    missing = sorted(set(sweep["chosen"]) - set(stats_rows))
    assert not missing, "shapes choose statistics kernels that are not built: %r" % missing
    unreachable = sorted(set(stats_rows) - set(sweep["chosen"]))
    assert not unreachable, "built statistics kernels no shape chooses: %r" % unreachable


def test_statistics_kernels_are_a_family_of_their_own_by_name(built):
    """the frozen tests find the fast kernels by `ladder_wu_kernelI` / `ladder_colour_kernelI` in the mangled name and by labels that start with
    `wave<` / `colour<`: a statistics kernel matches neither, and lives in a translation unit of its own"""
    stats_rows, rows = built
    assert len(stats_rows) == 28
    for r in stats_rows.values():
        assert "ladder_wu_kernelI" not in r["kernel"] and "ladder_colour_kernelI" not in r["kernel"] and "ladder_kernelI" not in r["kernel"], r
        assert r["unit"] in ("ladder_wu_stats", "ladder_wu_stats_alpha", "ladder_colour_stats"), r
    for r in rows:
        if r["unit"] in ("ladder_wu_stats", "ladder_wu_stats_alpha", "ladder_colour_stats"):
            assert r["label"] in stats_rows, r                            # ... which holds nothing else


def test_statistics_kernels_use_no_scratch_within_128_vgprs(built):
    stats_rows, _ = built
    for lab, r in sorted(stats_rows.items()):
        print("%-52s VGPRs %3d  SGPRs %3d  scratch %d  occupancy %d" % (lab, r["VGPRs"], r["SGPRs"], r["ScratchSize"], r["Occupancy"]))
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 128 and r["Occupancy"] >= 4, r


def test_a_statistics_launch_replays_the_cascade(T):
    """wave_cascade_once() (what a launch puts into LadderArgs::wu_once) is false for a statistics launch at the shapes where the fast kernel walks the
    cascade once per workgroup: under STATS every wave decides the pair below its own slot"""
    from qecmc import _lib as L_
    dims, msg = np.zeros(len(FIELDS), dtype=np.int32), C.create_string_buffer(600)
    pr = L_.make_params(p=0.1, eta=3.0, alpha=1.5, iters=10, steps=10, code=0, L=9, Nc=2, noise=0, scan=3)
    assert T.qt_plan_dims(C.byref(pr), dims.ctypes.data, msg, len(msg)) == 0, msg.value
    rows = []
    for Nc, stats in itertools.product((5, 6, 7), (0, 1)):
        s = dict(zip(FIELDS, (int(x) for x in dims)))
        s.update(Nc=Nc, top_acc=1, lower_acc=0, logical=1, conv=0, queue=0, uset=0, xyz=0, stats=stats, resume=0, neff=0, f32ok=0, swap_fast_ok=1, iters=10, tune=0)
        rows.append([s[f] for f in FIELDS])
    shapes = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros(len(shapes), dtype=np.int32)
    T.qt_wave_cascade_once(shapes.ctypes.data, len(shapes), out.ctypes.data)
    assert [int(x) for x in out] == [1, 0] * 3
    keys = keys_of(T, shapes)
    assert [int(k[4]) for k in keys] == [0, KEY_STATS] * 3 and all(int(k[0]) == 2 for k in keys)
