"""The words of the list makers, the part of their host frame that needs no GPU: rs-vgaligner_amd/csrc/vga_oplist_text.hpp compiled
for the host alone.  The entry points of coverage, the pileup and the insertion table build their error texts from these formats
and their own name; every string the library could hand out before is listed here as a literal and must come out byte for
byte."""
import ctypes as C
import os
import subprocess

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")

HARNESS = r"""
#include <cstdio>
#include <cstring>
#include "vga_oplist_text.hpp"
static const oplist_text *const T[3] = {&OPLIST_TEXT_COV, &OPLIST_TEXT_PU, &OPLIST_TEXT_IA};
extern "C" {
const char *t_field(int m, int f) {
    const oplist_text &t = *T[m];
    const char *const v[7] = {t.name, t.who, t.what, t.list, t.mark, t.refusal, t.limit};
    return v[f];
}
const char *t_paths_refusal() { return OPLIST_REFUSAL_PATHS; }
// what: 0 no index, 1 too large, 2 no memory, 3 reserve, 4 off, 5 wrapped, 6 no list, 7 refused, 8 wide
void t_format(int what, int m, const char *fn, const char *s, unsigned long long n, unsigned flags, char *out, size_t cap) {
    const oplist_text &t = *T[m];
    switch (what) {
    case 0: snprintf(out, cap, OPLIST_ERR_NO_INDEX, fn); break;
    case 1: snprintf(out, cap, OPLIST_ERR_TOO_LARGE, fn, t.limit); break;
    case 2: snprintf(out, cap, OPLIST_ERR_NO_MEMORY, fn); break;
    case 3: snprintf(out, cap, OPLIST_ERR_RESERVE, fn, s); break;
    case 4: snprintf(out, cap, OPLIST_ERR_OFF, fn, t.name); break;
    case 5: snprintf(out, cap, OPLIST_ERR_WRAPPED, fn, n); break;
    case 6: snprintf(out, cap, OPLIST_ERR_NO_LIST, t.who, (size_t)n, t.what, flags); break;
    case 7: snprintf(out, cap, OPLIST_ERR_REFUSED, s); break;
    case 8: snprintf(out, cap, OPLIST_ERR_WIDE, fn); break;
    }
}
}
"""

COV, PU, IA = 0, 1, 2
NO_INDEX, TOO_LARGE, NO_MEMORY, RESERVE, OFF, WRAPPED, NO_LIST, REFUSED, WIDE = range(9)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("oplist_text")
    src, so = d / "harness.cpp", d / "harness.so"
    src.write_text(HARNESS)
    # (a host compiler alone: the header names no HIP type and calls no HIP function; -Wformat checks every format against its arguments)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wformat=2", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.t_field.restype, L.t_field.argtypes = C.c_char_p, [C.c_int, C.c_int]
    L.t_paths_refusal.restype = C.c_char_p
    L.t_format.restype = None
    L.t_format.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_ulonglong, C.c_uint, C.c_char_p, C.c_size_t]
    return L


def fmt(lib, what, m, fn="", s="", n=0, flags=0):
    out = C.create_string_buffer(512)
    lib.t_format(what, m, fn.encode(), s.encode(), n, flags, out, len(out))
    return out.value.decode()


def test_what_the_makers_are_called(lib):
    """trace names of the lists, the lines of the align trace, and who / what of a winner without a list"""
    want = {COV: ("coverage", "coverage", "run", "run list", "coverage"), PU: ("pileup", "pileup", "event", "pileup list", "pileup"),
            IA: ("insertion", "insertions", "insertion", "insertion list", "insertions")}
    for m, fields in want.items():
        assert tuple(lib.t_field(m, f).decode() for f in range(5)) == fields
    assert fmt(lib, NO_LIST, COV, n=3, flags=2) == "coverage: reported alignment 3 has no run list (flags 2)"
    assert fmt(lib, NO_LIST, PU, n=0, flags=0) == "pileup: reported alignment 0 has no event list (flags 0)"
    assert fmt(lib, NO_LIST, IA, n=12, flags=6) == "insertions: reported alignment 12 has no insertion list (flags 6)"


def test_host_route_refusals(lib):
    tail = " under VGA_SUBGRAPH=host (the subgraph handles are then on the host only)"
    want = {COV: "vga_align_batch: read coverage is not counted" + tail, PU: "vga_align_batch: the pileup is not counted" + tail,
            IA: "vga_align_batch: the inserted letters are not counted" + tail}
    for m, text in want.items():
        assert fmt(lib, REFUSED, m, s=lib.t_field(m, 5).decode()) == text
    assert fmt(lib, REFUSED, COV, s=lib.t_paths_refusal().decode()) == "vga_align_batch: path support is not scored" + tail


def test_begin_errors(lib):
    assert [fmt(lib, NO_INDEX, m, fn) for m, fn in ((COV, "vga_coverage_begin"), (PU, "vga_pileup_begin"), (IA, "vga_insertion_begin"))] == [
        "vga_coverage_begin: no index uploaded", "vga_pileup_begin: no index uploaded", "vga_insertion_begin: no index uploaded"]
    assert [fmt(lib, TOO_LARGE, m, fn) for m, fn in ((COV, "vga_coverage_begin"), (PU, "vga_pileup_begin"), (IA, "vga_insertion_begin"))] == [
        "vga_coverage_begin: graph too large for 32-bit positions", "vga_pileup_begin: graph too large for 29-bit positions",
        "vga_insertion_begin: graph too large for 26-bit positions"]
    assert fmt(lib, NO_MEMORY, COV, "vga_coverage_begin") == "vga_coverage_begin: out of host memory"
    assert fmt(lib, NO_MEMORY, COV, "vga_path_support_begin") == "vga_path_support_begin: out of host memory"   # (the run lists' other reader)
    assert fmt(lib, NO_MEMORY, PU, "vga_pileup_begin") == "vga_pileup_begin: out of host memory"
    assert fmt(lib, NO_MEMORY, IA, "vga_insertion_begin") == "vga_insertion_begin: out of host memory"
    assert fmt(lib, RESERVE, PU, "vga_pileup_begin", s="out of memory") == "vga_pileup_begin: out of memory"


def test_counting_is_off(lib):
    want = {(COV, "vga_coverage_reset"): "vga_coverage_reset: counting is off (vga_coverage_begin)",
            (COV, "vga_coverage_read"): "vga_coverage_read: counting is off (vga_coverage_begin)",
            (PU, "vga_pileup_reset"): "vga_pileup_reset: counting is off (vga_pileup_begin)",
            (PU, "vga_pileup_read"): "vga_pileup_read: counting is off (vga_pileup_begin)",
            (PU, "vga_variant_call"): "vga_variant_call: counting is off (vga_pileup_begin)",
            (IA, "vga_insertion_reset"): "vga_insertion_reset: counting is off (vga_insertion_begin)",
            (IA, "vga_insertion_read"): "vga_insertion_read: counting is off (vga_insertion_begin)",
            (IA, "vga_insertion_call"): "vga_insertion_call: counting is off (vga_insertion_begin)"}
    for (m, fn), text in want.items():
        assert fmt(lib, OFF, m, fn) == text


def test_wrapped_and_wide_counters(lib):
    n = 0xFFFFFFFF
    for m, fn in ((COV, "vga_coverage_read"), (PU, "vga_pileup_read"), (PU, "vga_variant_call"), (IA, "vga_insertion_read"), (IA, "vga_insertion_call")):
        assert fmt(lib, WRAPPED, m, fn, n=n) == fn + ": 4294967295 alignments counted: a 32-bit counter may have wrapped"
    assert fmt(lib, WRAPPED, PU, "vga_pileup_read", n=2**33 + 5) == "vga_pileup_read: 8589934597 alignments counted: a 32-bit counter may have wrapped"
    for fn in ("vga_variant_call", "vga_variant_call_table", "vga_insertion_call", "vga_insertion_call_table"):
        assert fmt(lib, WIDE, PU, fn) == fn + ": a counter of 2^40 or more"
