"""The barriers of a ladder step of the headline scan = wave kernel, counted in the compiler's ISA (no GPU): tools/wave_step_segments.py follows the paths
round each role's step loop of ladder_wu_kernel<512,8,toric,12 words,iters 10> and cuts them at their s_barrier instructions.  Since the walked forms
publish their records in front of the first barrier (csrc/ladder_wu.hpp, kWuStepBarriers == 2) a step has two barriers on every path: on the walked one,
where the waves below the top draw the next step's acceptance block BETWEEN the two, and on the replay's, which keeps its step -- state stores and record
between the two barriers, the draw behind the second.  The paths are told apart by what stands between the barriers, never by a count: the test pins the
barrier numbers alone and prints the instruction counts it found."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc-qec-toric-rl_amd", "csrc")
KERNEL = "ladder_wu_kernelILi512ELi8ELi0ELi12ELb0ELb0ELi10ELb0E"


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    """every distinct path the tool can follow round each role's loop: the common one and, one at a time, each rare block kept (--keep k)"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("isa") / "ladder_wu.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, "ladder_wu.hip"], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    spec = importlib.util.spec_from_file_location("wave_step_segments", os.path.join(ROOT, "tools", "wave_step_segments.py"))
    seg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(seg)
    ins, labels, headers, member = seg.parse(seg.kernel_body(out, KERNEL))
    found = {}
    for h in headers:
        for keep in [()] + [(k,) for k in range(1, 41)]:
            ops = []
            counts = seg.walk(ins, labels, member, h, 40, keep, False, ops)
            if counts and len(counts) >= 3:
                found.setdefault(h, {}).setdefault(tuple(counts), (keep, ops))
    return found


def _draws(stretch):
    """a Philox block stands in the stretch: its 32 x 32 -> 64 bit products on lane-varying counters"""
    return any(o.startswith("v_mul_hi_u32") or o.startswith("v_mad_u64_u32") for o in stretch)


def _stores(stretch):
    return sum(o.startswith("ds_write") for o in stretch)


def test_every_path_of_a_step_has_two_barriers(paths):
    assert len(paths) == 2, "the two roles' step loops: %r" % sorted(paths)
    for h, ps in paths.items():
        for counts, (keep, ops) in ps.items():
            print("%s --keep %-4s barriers %d  last barrier -> first %d  between %s  (stores %s)" % (
                h, ",".join(map(str, keep)) or "-", len(counts) - 1, counts[0] + counts[-1], list(counts[1:-1]), [_stores(o) for o in ops[1:-1]]))
            assert len(counts) - 1 == 2, (h, keep, counts)


def test_the_lower_roles_walked_path_draws_between_its_two_barriers_and_the_replay_keeps_its_step(paths):
    # the role of the waves below the top: the loop in which some path draws between the barriers (the top role draws in front of the first one)
    lower = [h for h, ps in paths.items() if any(_draws(ops[1]) for _, ops in ps.values())]
    assert len(lower) == 1, lower
    walked = [(c, k) for c, (k, ops) in paths[lower[0]].items() if _draws(ops[1])]
    replay = [(c, k) for c, (k, ops) in paths[lower[0]].items() if not _draws(ops[1])]
    assert walked and replay
    for counts, keep in walked:
        ops = paths[lower[0]][counts][1]
        print("walked --keep %s: %s" % (keep, counts))
        assert len(counts) - 1 == 2
        assert _stores(ops[1]) >= 12 and _stores(ops[0]) + _stores(ops[2]) >= 1        # the state stores behind B1, the record in front of it
    for counts, keep in replay:
        ops = paths[lower[0]][counts][1]
        print("replay --keep %s: %s" % (keep, counts))
        assert len(counts) - 1 == 2
        assert _stores(ops[1]) >= 13 and _draws(ops[2])                               # stores and record between B1 and B2, the draw behind B2
