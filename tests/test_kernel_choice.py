"""Which kernel every launch runs, on the CPU: csrc/kernel_choice.hpp choose_kernel(), compiled alone by g++ (make tables), over every
shape the C-ABI accepts -- each code, rule and scan over the L of which validate_params() and plan_host() (csrc/plan_host.hpp, asked with real
parameter blocks) make plans, Nc = 1 .. 16, every noise / scan / conv / queue / stats / uset / resume
combination a plan or a launch can present, the temperature ladders' accept-all and swap-threshold bits, iters 10 / another one within
and one beyond what scan = wave is built for, and all 8 combinations of the developer bits the choice reads.

  (a) every kernel chosen is built (csrc/build/*.res), and the shapes no kernel is built for are refused for a named reason;
  (b) every ladder / wave / colour kernel in the build is chosen by at least one shape (what none chooses is not built);
  (c) the kernels of BASELINE configurations 2-5 at the shapes `bench.py --config N` resolves to by default;
  (d) what plan_host() itself says of the sweep: which of its blocks get no plan and why, the ladders its plans present, the persistent grid."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

from hostlib import KERNEL_SHAPE_FIELDS as FIELDS
from hostlib import ROTATED, TORIC, XZZX, resource_rows, tables_lib
from qecmc import _lib as L_

CODES = ["toric", "xzzx", "rotated", "planar"]
FLAGS = ["conv", "gsplit", "biased", "scan", "gentop", "uset", "alpha", "pre", "delut", "queue", "ssw"]   # LadderFlag bit order

# the kernels of BASELINE configurations 2-5 (bench.py CONFIGS, --scan auto, iters 10, p_logical 0.5, fixed length), and -- bench.py --full
# beside a scan = wave line -- the scan = 0 kernel on the same batch
BASELINE = {
    "config 2": (dict(code=TORIC, L=9, Nc=8, scan=3), "wave<512,8,toric: 12 words, iters 10>"),
    "config 2, scan = 0": (dict(code=TORIC, L=9, Nc=8, scan=0), "ladder<512,8,toric: gsplit|delut|ssw>"),
    "config 3": (dict(code=TORIC, L=15, Nc=8, scan=3), "wave<512,6,toric: 32 words, iters 10>"),
    "config 3, scan = 0": (dict(code=TORIC, L=15, Nc=8, scan=0), "ladder<512,4,toric: pre|delut>"),
    "config 4": (dict(code=XZZX, L=9, Nc=8, scan=0, noise=1), "ladder<512,8,xzzx: biased|gentop|ssw>"),
    "config 5": (dict(code=ROTATED, L=21, Nc=8, scan=0), "ladder<512,4,rotated: gentop|pre|delut>"),
}
# why a shape the C-ABI accepts has no kernel (kernel_choice.hpp refuse()): each reason is met by some shape, and no other
REFUSALS = {
    "work queue offered to a shape without queue kernels",
    "uset: depolarizing or alpha rule, random scan, fixed length, no logical moves",
    "uset: Chain_xyz runs single chains of the table-driven codes",
    "uset, alpha rule: single chains of the xzzx / rotated codes",
    "uset: not with scan = colour",
    "scan = colour: no resumed ladders",
    "scan = wave: outside what it is built for",
}


@pytest.fixture(scope="module")
def T():
    return tables_lib()          # (qt_choose_kernels, qt_plan_dims and qt_plan get their signatures there)


def label(key):
    """a kernel as tools/kernel_resources.py labels it ("ladder<512,8,toric: gsplit|delut|ssw>", "wave<512,8,toric: 12 words, iters 10>"; the
    colour kernels "colour<1024,4,xzzx: rule 1, conv>"), or "refused: <why>" """
    family, maxt, minw, code, flags, wv, conv, it, alpha, rule, why = (int(x) for x in key)
    if family == 1:
        return "ladder<%d,%d,%s: %s>" % (maxt, minw, CODES[code], "|".join(n for i, n in enumerate(FLAGS) if flags >> i & 1) or "plain")
    if family == 2:
        return "wave<%d,%d,%s: %d words%s%s%s>" % (maxt, minw, CODES[code], wv, ", conv, queue" if conv else "", ", alpha" if alpha else "",
                                                 ", iters %d" % it if it else "")
    if family == 3:
        return "colour<%d,%d,%s: rule %d%s>" % (maxt, minw, CODES[code], rule, ", conv" if conv else "")
    return "refused: " + C.string_at(why).decode()


def choose(T, shapes):
    """{label: number of shapes} of an int32 array [n][len(FIELDS)] of shapes"""
    shapes = np.ascontiguousarray(shapes, dtype=np.int32)
    keys = np.zeros((len(shapes), 11), dtype=np.int64)
    T.qt_choose_kernels(shapes.ctypes.data, len(shapes), keys.ctypes.data)
    rows, first, counts = np.unique(keys.view(np.dtype((np.void, 88))).ravel(), return_index=True, return_counts=True)
    return {label(keys[i]): int(n) for i, n in zip(first, counts)}


def params(**kw):
    """a real parameter block (qecmc_params): p, eta and alpha inside every rule's range unless given"""
    return L_.make_params(**dict(dict(p=0.1, eta=3.0, alpha=1.5, iters=10, steps=10), **kw))


def plan_dims(T, pr):
    """validate_params() and the first phase of plan_host() (csrc/plan_host.hpp) on a parameter block: (rc, message, the shape's static fields)"""
    shape, msg = np.zeros(len(FIELDS), dtype=np.int32), C.create_string_buffer(600)
    rc = T.qt_plan_dims(C.byref(pr), shape.ctypes.data, msg, len(msg))
    return rc, msg.value.decode(), dict(zip(FIELDS, (int(x) for x in shape)))


def plan(T, pr, cu_count=1):
    """validate_params() and plan_host() on a parameter block: (rc, message, the plan's shape, lds_bytes, the persistent grid on cu_count CUs)"""
    shape, msg, lds, grid = np.zeros(len(FIELDS), dtype=np.int32), C.create_string_buffer(600), C.c_uint64(), C.c_uint32()
    rc = T.qt_plan(C.byref(pr), cu_count, shape.ctypes.data, C.byref(lds), C.byref(grid), msg, len(msg))
    return rc, msg.value.decode(), dict(zip(FIELDS, (int(x) for x in shape))), lds.value, grid.value


def code_shape(T, code, L, noise, scan):
    """the static fields of the shape of the plans of (code, L, rule, scan), or None where the library makes no plan of them: validate_params()
    refuses the block (asked with a two-rung ladder without logical moves, which no rule about Nc or p_logical objects to) or the generator
    table exceeds its LDS bound"""
    rc, _, dims = plan_dims(T, params(code=code, L=L, Nc=2, noise=noise, scan=scan))
    return None if rc else {f: dims[f] for f in ("code", "noise", "scan", "L", "W", "nq", "ncls", "n_gen", "n_types", "gen_type")}


def blocks(T):
    """the static shape fields of every code, rule, scan and L the library makes plans of"""
    for code, noise, scan, L in itertools.product(range(4), range(3), range(4), range(0, 70)):
        base = code_shape(T, code, L, noise, scan)
        if base is not None:
            yield base


def launch_modes(scan):
    """(conv, queue, uset, xyz, stats, resume) a launch presents: qecmc_pteq_launch_dev (a criterion run takes the plan's work queue
    unless it asks for final states or statistics), qecmc_pteq_resume_dev / qecmc_ladder_step (resume), the unique-chain estimators (uset)"""
    for conv in (0, 1):
        for stats in ((0, 1) if scan in (0, 1) else (0,)):
            yield conv, 0, 0, 0, stats, 0
        if conv and scan == 0:
            yield conv, 1, 0, 0, 0, 0
        for xyz in (0, 1):
            yield conv, 0, 1, xyz, 0, 0
    yield 0, 0, 0, 0, 0, 1


def ladders(noise, scan, Nc):
    """(top_acc, lower_acc, swap_fast_ok, f32ok) of the plan's temperature ladders: the depolarizing rule's top rung at p = 0.75 (every
    rung there when p = 0.75; p so close below it that p_diff > 1 - 2^-32 loses swap_fast_ok while the lower rungs still test, tests/range_cases.py
    group A), none under the table-driven rules (the colour scan's alpha top rung takes the coin); bias_f32ok either way"""
    if noise == 0:
        return [(int(Nc >= 2), 0, 1, int(Nc == 1)), (1, int(Nc >= 2), int(Nc == 1), int(Nc == 1))] + ([(1, 0, 0, 0)] if Nc >= 2 else [])
    top = int(noise == 2 and scan == 2 and Nc >= 2)
    return [(top, 0, 1, f) for f in (0, 1)]


def all_shapes(T):
    """every shape, in blocks of one code, L, rule and scan"""
    for base in blocks(T):
        noise, scan, rows = base["noise"], base["scan"], []
        for Nc in range(1, 17):
            for (top, lower, sfo, f32), (conv, queue, uset, xyz, stats, resume), logical, iters, tune in itertools.product(
                    ladders(noise, scan, Nc), launch_modes(scan), (0, 1), (10, 7, 200), range(0, 16, 2)):
                s = dict(base, Nc=Nc, top_acc=top, lower_acc=lower, swap_fast_ok=sfo, f32ok=f32, conv=conv, queue=queue, uset=uset, xyz=xyz,
                         stats=stats, resume=resume, neff=int(resume and noise == 2), logical=logical, iters=iters, tune=tune)
                rows.append([s[f] for f in FIELDS])
        yield np.array(rows, dtype=np.int32)


def built_kernels():
    """label -> row of every ladder / wave / colour kernel in csrc/build/*.res"""
    out = {}
    for r in resource_rows():
        m = re.search(r"ladder_colour_kernelILi(\d+)ELb([01])ELi(\d+)ELi(\d+)ELi(\d+)E", r["kernel"])
        if m:   # ladder_colour_kernel<CODE, CONV, RULE, MAXT, MINW>
            code, conv, rule, maxt, minw = (int(x) for x in m.groups())
            r = dict(r, label="colour<%d,%d,%s: rule %d%s>" % (maxt, minw, CODES[code], rule, ", conv" if conv else ""))
        if r["label"].startswith(("ladder<", "wave<", "colour<")):
            out[r["label"]] = r
    return out


@pytest.fixture(scope="module")
def sweep(T):
    """one pass over all_shapes(): label -> number of shapes that choose it ("refused: why" for the shapes without a kernel), and the pass's size"""
    seen, n_blocks = {}, 0
    for block in all_shapes(T):
        n_blocks += 1
        for lab, n in choose(T, block).items():
            seen[lab] = seen.get(lab, 0) + n
    return dict(chosen=seen, shapes=sum(seen.values()), blocks=n_blocks)


@pytest.fixture(scope="module")
def chosen(sweep):
    return sweep["chosen"]


def test_the_sweep_is_as_large_as_it_was(sweep):
    # what all_shapes() yielded while it restated validate_params and build_plan in Python: taking the enumeration from plan_host() must not shrink it
    # (8 143 872 until the depolarizing rule gained the ladder just below p = 0.75: swap_fast_ok off, the lower rungs still testing)
    assert (sweep["shapes"], sweep["blocks"]) == (10662432, 644)


# what validate_params() / plan_host() answer to the (code, L, rule, scan, Nc) of the sweep that get no plan: the sweep is a superset of the plans,
# and the chooser answers for all of it
PLAN_REFUSALS = {
    "wave, one rung": r"^scan = wave needs a ladder whose top rung sits at p = 0\.75 \(Nc >= 2\)$",
    "colour, one rung, logical moves": r"^scan = colour needs the top rung at p = 0\.75 \(Nc >= 2\) when logical moves are on$",
    "table-driven rules, nq > 511": r"^biased / alpha noise packs the error counts in 10-bit fields: nq=\d+$",
    "LDS": r"^L=\d+ Nc=\d+ needs \d+ B of LDS per workgroup \(> 160 KiB\)$",
    "LDS, colour": r"^scan = colour: L=\d+ Nc=\d+ needs \d+ B of LDS per workgroup \(> 160 KiB\)$",
    "wave, not built": r"^scan = wave: L=\d+ Nc=\d+ p=0\.1 is outside what it is built for \(depolarizing rule: a top rung that accepts every move, at most 16 packed",
}


def test_plans_refused_within_the_sweep(T):
    met, n = {}, 0
    for base in blocks(T):
        for Nc in range(1, 17):
            rc, msg, shape, lds, _ = plan(T, params(code=base["code"], L=base["L"], noise=base["noise"], scan=base["scan"], Nc=Nc, p_logical=0.5))
            n += 1
            if rc == 0:
                assert {f: shape[f] for f in base} == base and shape["Nc"] == Nc and 0 < lds <= 160 * 1024
                continue
            # (the colour kernel's LDS holds what build_plan once tested first, states + records + histogram, and more: far from 160 KiB at every
            # colour shape of the sweep, that first test never answered before the colour kernel's own)
            assert base["scan"] != 2 or 4 * (Nc * base["W"] + 4 * Nc + base["ncls"]) <= 160 * 1024
            why = [name for name, rx in PLAN_REFUSALS.items() if re.search(rx, msg)]
            assert rc == -4 and len(why) == 1, msg
            met[why[0]] = met.get(why[0], 0) + 1
    assert n == 644 * 16
    for name, k in sorted(met.items()):
        print("%5d of %d (code, L, rule, scan, Nc) refused: %s" % (k, n, name))
    assert set(met) == set(PLAN_REFUSALS)


@pytest.mark.parametrize("kw", [dict(code=TORIC, L=5, noise=0, p=0.1), dict(code=TORIC, L=5, noise=0, p=0.75), dict(code=TORIC, L=5, noise=0, p=0.75 - 1e-11),
                                dict(code=ROTATED, L=5, noise=0, p=0.1),
                                dict(code=XZZX, L=5, noise=1, eta=3.0, iters=10), dict(code=XZZX, L=5, noise=1, eta=1e6, iters=400),
                                dict(code=XZZX, L=5, noise=1, eta=3.0, iters=1000), dict(code=ROTATED, L=5, noise=2, alpha=1.5, iters=10),
                                dict(code=ROTATED, L=5, noise=2, alpha=6.0, iters=128), dict(code=XZZX, L=5, noise=2, alpha=1.5, iters=600)])
def test_plans_present_the_ladders_the_sweep_claims(T, kw):
    """ladders(): (top_acc, lower_acc, swap_fast_ok, f32ok) of a real plan is one of the tuples the sweep runs for its rule, scan and Nc -- the
    depolarizing ladders (p below 0.75, so close below it that a swap threshold leaves 32 bits, and at 0.75), the table-driven rules on each side of the single-precision bound (4 iters max|log2 ratio| <= 2000,
    iters <= 512), the alpha rule's accept-all top rung on scan = colour"""
    seen = set()
    for scan, Nc in itertools.product(range(4), (1, 2, 8)):
        rc, msg, shape, _, _ = plan(T, params(scan=scan, Nc=Nc, **kw))
        if rc == 0:
            got = tuple(shape[f] for f in ("top_acc", "lower_acc", "swap_fast_ok", "f32ok"))
            assert got in ladders(kw["noise"], scan, Nc), (scan, Nc, got)
            seen.add(got[3])
    assert seen       # (some scan and Nc of every case makes a plan)


def test_every_chosen_kernel_is_built_and_every_refusal_is_named(chosen):
    built = built_kernels()
    kernels = {k for k in chosen if not k.startswith("refused: ")}
    assert len(kernels) > 100
    missing = sorted(kernels - set(built))
    assert not missing, "shapes choose kernels that are not built: %r" % missing
    assert {k[len("refused: "):] for k in chosen if k.startswith("refused: ")} == REFUSALS


def test_every_built_kernel_is_chosen(chosen):
    unreachable = sorted(set(built_kernels()) - set(chosen))
    assert not unreachable, "built kernels no shape chooses (remove them from their unit's list): %r" % unreachable


def bench_shape(T, code, L, Nc, scan, noise=0):
    s = dict(code_shape(T, code, L, noise, scan), Nc=Nc, top_acc=int(noise == 0), lower_acc=0, logical=1, conv=0, queue=0, uset=0, xyz=0, stats=0,
             resume=0, neff=0, f32ok=0, swap_fast_ok=1, iters=10, tune=0)
    return [s[f] for f in FIELDS]


@pytest.mark.parametrize("name", sorted(BASELINE))
def test_baseline_kernels(T, name):
    kw, want = BASELINE[name]
    assert list(choose(T, [bench_shape(T, **kw)])) == [want]


def test_queue_grid_waves_per_cu(T):
    # the persistent grid of a work-queue plan (plan_host.hpp) holds 4 SIMDs x MINW waves of the kernel chosen with the queue offered: 8 per
    # SIMD for the 512-thread depolarizing ladder kernels, 4 for the 1024-thread ones and the biased / alpha queue kernels; scan = wave 8, 6 from 13
    # words on and for the alpha rule's criterion kernels -- or as many workgroups as their LDS lets a CU hold, if that is fewer, and at least one
    def waves(**kw):
        s = bench_shape(T, **{k: kw[k] for k in ("code", "L", "Nc", "scan", "noise") if k in kw})
        for k, v in dict({k: v for k, v in kw.items() if k in ("top_acc", "f32ok", "logical")}, conv=1, queue=1).items():
            s[FIELDS.index(k)] = v
        keys = np.zeros(11, dtype=np.int64)
        T.qt_choose_kernels(np.array(s, dtype=np.int32).ctypes.data, 1, keys.ctypes.data)
        family, minw, flags, conv = keys[0], keys[2], keys[4], keys[6]
        per_cu = 4 * minw // s[FIELDS.index("Nc")] if (family == 1 and flags & 512) or (family == 2 and conv) else 0
        # ... and what the plan of such a parameter block says itself, on a device of one CU
        rc, msg, _, lds, grid = plan(T, params(code=kw["code"], L=kw["L"], Nc=kw["Nc"], scan=kw["scan"], noise=kw.get("noise", 0), conv_mode=1,
                                               p_logical=0.5 * kw.get("logical", 1)))
        assert rc == 0, msg
        assert grid == (max(1, min(per_cu, 160 * 1024 // lds)) if per_cu else 0)
        return per_cu
    assert waves(code=TORIC, L=9, Nc=8, scan=0) == 32 // 8 and waves(code=TORIC, L=9, Nc=12, scan=0) == 16 // 12
    assert waves(code=XZZX, L=9, Nc=8, scan=0, noise=1, top_acc=0) == 16 // 8
    assert waves(code=TORIC, L=9, Nc=8, scan=3) == 32 // 8 and waves(code=TORIC, L=11, Nc=4, scan=3) == 24 // 4
    assert waves(code=XZZX, L=5, Nc=5, scan=3, noise=2, top_acc=0, f32ok=1) == 24 // 5
    assert waves(code=TORIC, L=9, Nc=8, scan=0, logical=0) == 0          # no work queue without logical moves
