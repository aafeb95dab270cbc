"""The guarded arena and the table of tests/test_gpu_device_buffers.py, without a GPU: the arena reports a byte written next to a payload and
nothing else; the table names every entry point of include/qecmc.h that takes a hipStream_t (and the two qecmc_plan_set_* calls), passes every
nullable output in one row and NULL in another, routes every sampler launch row to a kernel the chooser builds, and every row's reference half
runs and is not vacuous (device_buffer_cases.conditions: conditions on the reference alone)."""
import os
import re

import numpy as np
import pytest

import device_buffer_cases as D
import guarded

HEADER = os.path.join(D.ROOT, "include", "qecmc.h")


# ------------------------------------------------------------------------------------------------------------------ the arena
@pytest.mark.parametrize("poison", [0x00, 0xA5])
def test_arena_reports_a_byte_next_to_a_payload_and_nothing_else(poison):
    arena = guarded.Arena("cpu", poison)
    ptr, view = arena.buf("out", 65 * 18, 18)                          # 65 rows of 18 bytes
    ptr_in, _ = arena.buf("in", 40, 4, dtype=np.int32, init=np.arange(10, dtype=np.int32))
    _, words = arena.buf("words", 65 * 4, 4, dtype=np.uint32)
    out, inp = arena["out"], arena["in"]
    assert ptr % 256 == 0 and ptr_in % 256 == 0 and ptr == out.whole.data_ptr() + out.guard
    assert out.whole.numel() == 2 * out.guard + 65 * 18
    assert out.guard == guarded.guard_bytes(18) == 4096 and out.guard >= 64 * 18
    assert guarded.guard_bytes(338) == 21760 and guarded.guard_bytes(338) % 256 == 0 and guarded.guard_bytes(338) >= 64 * 338
    assert view.numel() == 65 * 18 and words.numel() == 65 and (out.host() == poison).all() and (arena["words"].host() == poison * 0x01010101).all()
    assert np.array_equal(inp.host(), np.arange(10)) and arena.unchanged("in")
    assert arena.check() == []
    view[0] = poison ^ 0xFF; view[-1] = poison ^ 0xFF                  # inside the payload: not a guard's business
    assert arena.check() == []
    out.whole[out.guard + 65 * 18] = poison ^ 1                        # the byte just behind the payload
    bad = arena.check()
    assert len(bad) == 1 and bad[0].startswith("out: back guard, first byte at payload end + 0")
    out.whole[out.guard + 65 * 18] = poison
    out.whole[out.guard - 1] = poison ^ 1                              # ... and the one just before it
    inp.whole[-1] = poison ^ 0x80                                      # the far end of another buffer's back guard
    bad = arena.check()
    assert len(bad) == 2 and bad[0].startswith("out: front guard, first byte at payload - 1 ")
    assert bad[1].startswith("in: back guard, first byte at payload end + %d " % (inp.guard - 1))
    inp.view[3] = 77
    assert not arena.unchanged("in")


# ------------------------------------------------------------------------------------------------------------------ the header
def _prototypes():
    """name -> the parameter list of every `int qecmc_*(...)` of the header, and the comment block in front of it"""
    text = open(HEADER).read()
    out = {}
    for m in re.finditer(r"((?:/\*(?:[^*]|\*(?!/))*\*/\s*)*)\bint\s+(qecmc_\w+)\s*\(([^;{]*?)\)\s*;", text):
        out[m.group(2)] = (m.group(3), m.group(1))
    return out


def _stream_entry_points():
    return sorted(n for n, (params, _) in _prototypes().items() if "hip_stream" in params)


def _nullable(name):
    """the parameters of a prototype the header calls nullable: commented so in the prototype, or `name (nullable` in the comment block in front of it"""
    params, doc = _prototypes()[name]
    if not doc and name.endswith("_dev") and name[:-4] in _prototypes():                              # (the _dev form stands right behind its host form, under the same comment)
        doc = _prototypes()[name[:-4]][1]
    names = [re.sub(r"/\*.*?\*/", "", p).split()[-1].lstrip("*") for p in params.split(",")]
    marked = {re.sub(r"/\*.*?\*/", "", p).split()[-1].lstrip("*") for p in params.split(",") if re.search(r"/\*\s*nullable\s*\*/", p)}
    for word in re.findall(r"(\w+)\s*\(nullable", doc):
        marked |= {n for n in names if n == word or n == "d_" + word}
    return marked


def test_the_header_parser_finds_the_device_api():
    assert _stream_entry_points() == sorted([D.GENERATE, D.LIFT, D.CORRECT, D.LAUNCH, D.RESUME, D.RESUME_CONV])
    assert _nullable(D.LAUNCH) == {"d_tops0", "d_steps_done", "d_converged", "d_final_states", "d_workspace"}
    assert _nullable(D.GENERATE) == {"d_raw_out", "d_eq_true_out"}
    assert _nullable(D.LIFT) == {"d_status_out", "d_weight_out"}
    assert _nullable(D.CORRECT) == {"d_weight_out", "d_source_out", "d_moved_out", "d_status_out"}


def test_every_device_entry_point_has_a_row():
    named = {api for r in D.ROWS for api in r["api"]}
    for name in _stream_entry_points() + [D.SET_STATS, D.SET_SHORTEST]:
        assert name in _prototypes() and name in named, name
    assert named <= set(_prototypes())


def test_every_nullable_output_is_passed_in_one_row_and_null_in_another():
    for name in _stream_entry_points():
        rows = [r for r in D.ROWS if r["api"][0] == name]
        for param in _nullable(name):
            assert any(param in r["null"] for r in rows), (name, param, "is never NULL")
            assert any(param not in r["null"] for r in rows), (name, param, "is never passed")
        for r in rows:
            assert set(r["null"]) <= _nullable(name) | {"d_nerr_sums"}, r["name"]
    # (qecmc_plan_set_stats: "either nullable" -- d_nerr_sums needs d_swap_accepts, so that is the one that can be left out)
    stats = [r for r in D.ROWS if D.SET_STATS in r["api"]]
    assert any("d_nerr_sums" in r["null"] for r in stats) and any("d_nerr_sums" not in r["null"] for r in stats)


def test_the_rows_are_the_shapes_the_table_promises():
    launches = [r for r in D.ROWS if D.is_launch(r)]
    lanes = [r for r in launches if r["scan"] != "colour" and not r["queue_grid"] and r["replicas"] == 1]
    assert {r["N"] for r in lanes} == {1, 65}
    assert {r["N"] for r in launches if r["scan"] == "colour"} == {1, 3}
    assert all(r["first_syndrome"] % 64 == 0 for r in D.ROWS if r.get("scan") == "wave")
    assert all(r["N"] == 200 and not r["states"] for r in launches if r["queue_grid"])
    # final states wherever the entry point allows them: not on the work queue, not from the wave kernel's shortest-chain form
    for r in launches:
        if not r["states"]:
            assert r["queue_grid"] or "d_tops0" in r["null"] or (r["entry"] == "shortest") or (r["conv"] and r["replicas"] > 1), r["name"]
    for kind in ("generate", "lift", "corrections"):
        assert {r["N"] for r in D.ROWS if r["kind"] == kind} == {1, 65}


# ------------------------------------------------------------------------------------------------------------------ the rows
@pytest.mark.parametrize("name", [r["name"] for r in D.ROWS if D.is_launch(r)])
def test_the_chooser_picks_the_kernel_the_row_is_about(name):
    row = D.row_named(name)
    label = D.predicted(row)
    assert not label.startswith(("refused", "no plan", "no launch")), label
    assert all(e in label for e in row["expect"]), label


@pytest.mark.parametrize("name", D.NAMES)
def test_the_reference_half_runs_and_proves_something(name):
    row = D.row_named(name)
    ref = D.reference(name)
    assert D.conditions(row, ref) == []
    assert not any(v.flags.writeable for v in ref.values() if isinstance(v, np.ndarray))
