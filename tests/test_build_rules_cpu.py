"""What csrc/Makefile rebuilds when a header changes.  The Makefile lists no header: every compile leaves the compiler's own list (build/<output>.d) and
make reads it back.  The expectation here comes from the sources, not from the compiler: the closure of the quoted #include lines of each unit, .inc files
included.  After a build, `make -n -W <header>` must name exactly the units whose closure holds the header -- no stale object, and no unit rebuilt that
does not read it."""
import os
import re
import subprocess

import pytest

from hostlib import CSRC

HEADERS = ["ladder_wu.hpp", "ladder_colour.hpp", "class_sweep_ops.hpp", "corrections.hpp", "kernel_choice.hpp", "../../include/qecmc.h", "class_sample.hpp", "class_marginal.hpp",
           "class_minplus_tiled_trace.hpp"]
# a kernel family's header is read by its own unit and by the C-ABI host file, and by no other unit (class_marginal.hpp reads class_sample.hpp)
FAMILY = {"class_sample.hpp": {"capi.hip", "class_sample.hip", "class_marginal.hip"}, "class_marginal.hpp": {"capi.hip", "class_marginal.hip"},
          "class_minplus_tiled_trace.hpp": {"capi.hip", "class_minplus_tiled_trace.hip"}}


def closure(name, seen=None):
    """every file a source of csrc/ reaches through #include "..." lines, as paths relative to csrc/ (itself included)"""
    seen = set() if seen is None else seen
    if name not in seen:
        seen.add(name)
        text = open(os.path.join(CSRC, name), errors="replace").read()
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', text, re.M):
            path = os.path.normpath(os.path.join(os.path.dirname(name), inc))
            if os.path.exists(os.path.join(CSRC, path)):
                closure(path, seen)
    return seen


def units():
    line = re.search(r"^SRCS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    return line.split()


def would_rebuild(header, *goal):
    """the source files named by the commands make would run if `header` had just changed (None: as the tree stands)"""
    touched = ["-W", header] if header else []
    out = subprocess.run(["make", "-C", CSRC, "-n", *touched, *goal], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\b\w+\.(?:hip|cpp)\b", out))


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])          # a no-op when the library is built (build() ran)
    subprocess.check_call(["make", "-C", CSRC, "-s", "tables"])
    assert would_rebuild(None) == set() == would_rebuild(None, "tables")          # (up to date: only the header's change shows below)


def test_the_units_are_the_hip_files_of_csrc():
    assert sorted(units()) == sorted(f for f in os.listdir(CSRC) if f.endswith(".hip")) and len(units()) == 33


def test_no_unit_includes_an_inc():
    """a kernel family is a unit named after its header, never the tail of another unit: the two .inc files left are the kernel bodies their headers
    instantiate"""
    for u in units():
        assert not re.findall(r'^[ \t]*#[ \t]*include[ \t]*"[^"]+\.inc"', open(os.path.join(CSRC, u), errors="replace").read(), re.M), u
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".cpp")))
    readers = {inc: [f for f in names if re.search(r'#[ \t]*include[ \t]*"%s"' % re.escape(inc), open(os.path.join(CSRC, f), errors="replace").read())]
               for inc in sorted(f for f in os.listdir(CSRC) if f.endswith(".inc"))}
    assert readers == {"ladder_colour_body.inc": ["ladder_colour.hpp"], "ladder_wu_body.inc": ["ladder_wu.hpp"]}, readers


@pytest.mark.parametrize("header", HEADERS)
def test_a_header_rebuilds_exactly_the_units_that_read_it(built, header):
    want = {u for u in units() if header in closure(u)}
    assert want, header
    assert would_rebuild(header) == want
    if header in FAMILY:
        assert want == FAMILY[header]


def test_ladder_wu_hpp_rebuilds_the_eight_wave_units_and_nothing_else(built):
    assert would_rebuild("ladder_wu.hpp") == {u for u in units() if u.startswith("ladder_wu")}
    assert len(would_rebuild("ladder_wu.hpp")) == 8


def test_the_tables_library_follows_its_own_headers(built):
    reads = closure("tables_test_api.cpp")
    assert "class_sweep_ops.hpp" in reads and "ladder_wu.hpp" not in reads
    assert would_rebuild("class_sweep_ops.hpp", "tables") == {"tables_test_api.cpp"}
    assert would_rebuild("ladder_wu.hpp", "tables") == set()
