"""The launch decisions of the POA host, the parts that need no GPU: rs-vgaligner_amd/csrc/vga_poa_shape.hpp compiled for the host
alone -- the kernel family a call's penalties select, the LDS admission figure, and the launch shape (kernel, workgroup size,
LDS column window, LDS bytes) poa_choose_shape gives a sub-batch, by itself and under the environment switches
test_poa_paths_the_library_can_fall_back_to sets on the GPU."""
import ctypes as C
import os
import random
import subprocess

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
LDS_LIMIT = 160 * 1024 - 256
LDS, T4, T5, T6, T7 = range(5)  # poa_kernel; poa_family uses the first three
INSTANTIATED = {LDS: {128, 256, 512}, T4: set(range(128, 513, 64)) | {768, 1024}, T5: set(range(128, 513, 64)) | {768, 1024},
                T6: {64}, T7: {128, 256, 512, 1024}}
DEFAULT = (4, 2, 24, 1)
SWITCHES = ("VGA_POA_KERNEL", "VGA_POA_NT", "VGA_POA_WINDOW", "VGA_POA_T7_NT", "VGA_POA_T7_WINDOW", "VGA_POA_TB", "VGA_POA_ARENAS")

HARNESS = r"""
#include "vga_poa_shape.hpp"
static_assert(sizeof(tb_lds) == 6912, "what one wave of the traceback stages");
static vga_poa_params params_of(const int *g) {
    vga_poa_params p = {};
    p.match = 2; p.mismatch = 4; p.gap_open1 = g[0]; p.gap_ext1 = g[1]; p.gap_open2 = g[2]; p.gap_ext2 = g[3];
    return p;
}
extern "C" {
struct t_shape { int kernel, def_pen, nt, fam_nt; unsigned lds_cols, hg_cols, win_mask, fam_cols; unsigned long long lds, fam_lds; };
// the switches are read from the environment, as at the start of a call
int t_family(const int *gaps) { return (int)poa_choose_family(params_of(gaps), poa_read_switches()); }
int t_family_mm(const int *gaps, int match, int mismatch) {
    vga_poa_params p = params_of(gaps); p.match = match; p.mismatch = mismatch;
    return (int)poa_choose_family(p, poa_read_switches());
}
unsigned t_lds_cols(unsigned max_q) { return poa_lds_cols(max_q); }
unsigned long long t_min_lds(int family, unsigned max_q) { return poa_min_lds_bytes((poa_family)family, poa_lds_cols(max_q)); }
unsigned long long t_t5_bytes(unsigned hg_cols, unsigned lds_cols, int nt) { return poa_t5_lds_bytes(hg_cols, lds_cols, nt); }
int t_tb_fused() { return poa_read_switches().tb_fused; }
int t_arenas(unsigned long long *cap) { const poa_switches s = poa_read_switches(); *cap = s.has_arenas ? s.arenas : 0; return s.arenas_off; }
// flags: 1 giant, 2 general, 4 arena, 8 fused traceback
void t_shape_of(const int *gaps, unsigned max_q, double mean_w, double max_w, unsigned long long left, unsigned long long in_flight,
                unsigned n_cu, int flags, t_shape *o) {
    const poa_switches sw = poa_read_switches();
    poa_shape_in in;
    in.max_q = max_q; in.mean_w = mean_w; in.max_w = max_w; in.left = left; in.in_flight = in_flight; in.n_cu = n_cu;
    in.giant = flags & 1; in.general = flags & 2; in.arena = flags & 4; in.fused = flags & 8;
    in.default_penalties = gaps[0] == 4 && gaps[1] == 2 && gaps[2] == 24 && gaps[3] == 1;
    in.family = poa_choose_family(params_of(gaps), sw);
    const poa_shape s = poa_choose_shape(in, sw);
    o->kernel = s.kernel; o->def_pen = s.def_pen; o->nt = s.nt; o->fam_nt = s.fam_nt; o->lds_cols = s.lds_cols; o->hg_cols = s.hg_cols;
    o->win_mask = s.win_mask; o->fam_cols = s.fam_cols; o->lds = s.lds; o->fam_lds = s.fam_lds;
}
}
"""


class Shape(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kernel", "def_pen", "nt", "fam_nt")] + [(n, C.c_uint) for n in ("lds_cols", "hg_cols", "win_mask", "fam_cols")] + \
               [(n, C.c_ulonglong) for n in ("lds", "fam_lds")]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("poa_shape")
    src, so = d / "harness.cpp", d / "harness.so"
    src.write_text(HARNESS)
    # (a host compiler alone: the header names no HIP type and calls no HIP function)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    gaps = C.POINTER(C.c_int)
    L.t_family.restype, L.t_family.argtypes = C.c_int, [gaps]
    L.t_family_mm.restype, L.t_family_mm.argtypes = C.c_int, [gaps, C.c_int, C.c_int]
    L.t_lds_cols.restype, L.t_lds_cols.argtypes = C.c_uint, [C.c_uint]
    L.t_min_lds.restype, L.t_min_lds.argtypes = C.c_ulonglong, [C.c_int, C.c_uint]
    L.t_t5_bytes.restype, L.t_t5_bytes.argtypes = C.c_ulonglong, [C.c_uint, C.c_uint, C.c_int]
    L.t_tb_fused.restype = C.c_int
    L.t_arenas.restype, L.t_arenas.argtypes = C.c_int, [C.POINTER(C.c_ulonglong)]
    L.t_shape_of.restype = None
    L.t_shape_of.argtypes = [gaps, C.c_uint, C.c_double, C.c_double, C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_int, C.POINTER(Shape)]
    return L


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _gaps(g):
    return (C.c_int * 4)(*g)


def shape(L, max_q=10000, mean_w=2500.0, max_w=3500.0, left=10000, in_flight=0, n_cu=256, giant=False, general=False, arena=True,
          fused=True, gaps=DEFAULT):
    s = Shape()
    L.t_shape_of(_gaps(gaps), max_q, mean_w, max_w, left, in_flight, n_cu, giant | general << 1 | arena << 2 | fused << 3, C.byref(s))
    return s


def _window_is_sane(s):
    if s.win_mask == 0xFFFFFFFF:
        return s.hg_cols == s.lds_cols
    # (k_poa_dp_t7 always masks: "every column" is a power of two that holds them all)
    return s.hg_cols & (s.hg_cols - 1) == 0 and s.win_mask == s.hg_cols - 1 and (s.hg_cols < s.lds_cols or s.kernel == T7)


def test_family_is_decided_once_from_the_penalties(lib, monkeypatch):
    fam = lambda *g: lib.t_family(_gaps(g))
    assert fam(*DEFAULT) == T5
    assert fam(6, 3, 200, 1) == LDS            # o2 + e2 beyond k_poa_dp_t4's byte range
    assert fam(31, 32, 24, 1) == T5            # 4 (o1 + e1) <= 255
    assert fam(31, 33, 24, 1) == T4            # o1 + e1 == 64: k_poa_dp_t4's 4 g - 1 still fits a byte, k_poa_dp_t5's 4 g does not
    assert fam(32, 2, 24, 1) == T4 and fam(4, 2, 32, 1) == T4   # 4 o_k + 1 <= 128
    assert fam(4, 0, 24, 1) == LDS             # gap_ext1 == 0
    assert fam(1, 0, 60, 4) == LDS and fam(0, 1, 60, 4) == LDS  # o2 + e2 >= 64 beside o1 + e1 <= 1
    assert fam(10, 6, 24, 1) == T5             # (more than 8 bits for the two sums together is no reason for k_poa_dp_lds)
    assert lib.t_family_mm(_gaps(DEFAULT), 2, -3) == LDS and lib.t_family_mm(_gaps(DEFAULT), 1 << 19, 1 << 19) == LDS
    monkeypatch.setenv("VGA_POA_KERNEL", "t4")
    assert fam(*DEFAULT) == T4 and fam(6, 3, 200, 1) == LDS
    monkeypatch.setenv("VGA_POA_KERNEL", "unpacked")
    assert fam(*DEFAULT) == LDS
    monkeypatch.setenv("VGA_POA_KERNEL", "t6,generic")
    assert fam(*DEFAULT) == T5


def test_admission_is_computed_for_the_family_that_runs(lib):
    # k_poa_dp_lds keeps every column (7 B each): ~22 kbp.  k_poa_dp_t4 / t5 shrink their window to 512 columns: ~280 kbp
    assert lib.t_min_lds(LDS, 22000) <= LDS_LIMIT < lib.t_min_lds(LDS, 24000)
    for f in (T4, T5):
        assert lib.t_min_lds(f, 33000) <= LDS_LIMIT and lib.t_min_lds(f, 280000) <= LDS_LIMIT < lib.t_min_lds(f, 400000)
    # ... and what is admitted is what the smallest shape of the family needs
    for q in (100, 5000, 33000, 230000, 280000):
        cols = lib.t_lds_cols(q)
        assert cols % 16 == 0 and cols >= q + 17
        assert lib.t_t5_bytes(min(cols, 512), cols, 128) <= lib.t_min_lds(T5, q)


def test_default_launch_of_10_kbp_reads_with_wide_bands(lib):
    for left, in_flight in ((10000, 0), (2048, 2048), (40, 0)):
        s = shape(lib, left=left, in_flight=in_flight)
        assert s.kernel == T5 and s.def_pen == 1
        assert s.hg_cols == 4096 and s.win_mask == 4095 and s.lds_cols == lib.t_lds_cols(10000)
        assert s.lds <= LDS_LIMIT and s.nt in INSTANTIATED[T5]
        assert s.lds == lib.t_t5_bytes(4096, s.lds_cols, s.nt)
        assert (s.fam_nt, s.fam_cols, s.fam_lds) == (s.nt, s.hg_cols, s.lds)
    # 4096 columns let five workgroups share a CU
    assert 5 * (shape(lib).lds + 256) <= 160 * 1024
    # a query that fits a smaller array anyway keeps every column
    s = shape(lib, max_q=2500, mean_w=1200.0, max_w=1500.0)
    assert s.kernel == T5 and s.win_mask == 0xFFFFFFFF and s.hg_cols == s.lds_cols == lib.t_lds_cols(2500)
    # run-time penalties inside k_poa_dp_t5's range: the same kernel without the specialisation
    s = shape(lib, gaps=(5, 2, 24, 1))
    assert s.kernel == T5 and s.def_pen == 0


def test_narrow_bands_take_the_one_wave_kernel_in_chunk_pool_mode(lib):
    s = shape(lib, max_q=2500, mean_w=340.0, max_w=700.0)
    assert s.kernel == T6 and s.nt == 64 and s.lds <= LDS_LIMIT and s.def_pen == 1
    assert shape(lib, max_q=2500, mean_w=800.0, max_w=1000.0).kernel == T6
    assert shape(lib, max_q=2500, mean_w=800.0, max_w=1001.0).kernel == T5
    assert shape(lib, max_q=2500, mean_w=801.0, max_w=900.0).kernel == T5
    # what k_poa_dp_t6 hands back runs in k_poa_dp_t5: 128 threads, a window that just covers the widest estimated row
    g = shape(lib, max_q=2500, mean_w=340.0, max_w=700.0, general=True)
    assert g.kernel == T5 and g.nt == 128 and g.hg_cols == 1024 and g.win_mask == 1023
    assert shape(lib, max_q=2500, mean_w=340.0, max_w=300.0, general=True).hg_cols == 512
    # k_poa_dp_t6 needs chunk-pool mode and the fused traceback
    assert shape(lib, max_q=2500, mean_w=340.0, max_w=700.0, arena=False).kernel == T5
    assert shape(lib, max_q=2500, mean_w=340.0, max_w=700.0, fused=False).kernel == T5
    assert shape(lib, max_q=2500, mean_w=340.0, max_w=700.0, gaps=(31, 33, 24, 1)).kernel == T4


def test_giant_launch(lib):
    s = shape(lib, max_q=10000, mean_w=6000.0, max_w=9000.0, giant=True, left=12)
    assert s.kernel == T7 and s.nt == 1024 and s.lds <= LDS_LIMIT
    assert s.hg_cols >= s.lds_cols and s.hg_cols & (s.hg_cols - 1) == 0 and s.win_mask == s.hg_cols - 1   # every column
    # the k_poa_dp_t5 shape it starts from: 1 024 threads, every column
    assert s.fam_nt == 1024 and s.fam_cols == s.lds_cols
    # a query too long for that: the largest window that fits
    s = shape(lib, max_q=100000, mean_w=20000.0, max_w=60000.0, giant=True, left=3)
    assert s.kernel == T7 and s.nt == 1024 and s.lds <= LDS_LIMIT and s.hg_cols < s.lds_cols
    assert lib.t_t5_bytes(2 * s.hg_cols, s.lds_cols, 1024) > LDS_LIMIT
    # ... also where the giant shape is k_poa_dp_t5's or k_poa_dp_t4's (classic mode, a re-run): a window, halved until it fits
    for kw in ({"arena": False}, {"general": True}, {"gaps": (32, 2, 24, 1)}):
        s = shape(lib, max_q=65124, mean_w=20000.0, max_w=60000.0, giant=True, left=3, **kw)
        assert s.kernel in (T4, T5) and s.nt == 1024 and s.lds <= LDS_LIMIT and s.hg_cols == 16384 and s.win_mask == 16383
    # outside chunk-pool mode, or as a re-run, the giant shape is k_poa_dp_t5's
    for kw in ({"arena": False}, {"general": True}):
        s = shape(lib, max_q=10000, mean_w=6000.0, max_w=9000.0, giant=True, **kw)
        assert s.kernel == T5 and s.nt == 1024 and s.win_mask == 0xFFFFFFFF


def test_large_gap_penalties_give_the_fallback_kernel(lib):
    s = shape(lib, max_q=2500, gaps=(6, 3, 200, 1), arena=False, fused=False)
    assert s.kernel == LDS and s.nt in INSTANTIATED[LDS] and s.win_mask == 0xFFFFFFFF and s.def_pen == 0 and s.lds <= LDS_LIMIT
    # every column in LDS: the workgroup is halved until the rest fits beside them
    s = shape(lib, max_q=22000, gaps=(6, 3, 200, 1), arena=False, fused=False)
    assert s.kernel == LDS and s.lds <= LDS_LIMIT


@pytest.mark.parametrize("value, kernel", [("t4", T4), ("t5", T5), ("t6", T6), ("t6,generic", T6), ("t7", T7), ("t7,generic", T7), ("unpacked", LDS),
                                           ("generic", None), ("128", None), ("256", None), ("512", None)])
def test_kernel_switch(lib, monkeypatch, value, kernel):
    """VGA_POA_KERNEL as test_poa_paths_the_library_can_fall_back_to documents it, on a launch of 2.5 kbp reads with wide bands
    and on one with narrow bands"""
    monkeypatch.setenv("VGA_POA_KERNEL", value)
    wide = shape(lib, max_q=2500, mean_w=1200.0, max_w=1500.0)
    narrow = shape(lib, max_q=2500, mean_w=340.0, max_w=700.0)
    if kernel is None:
        assert wide.kernel == T5 and narrow.kernel == T6
    elif value == "t5":
        assert wide.kernel == T5 and narrow.kernel == T5   # k_poa_dp_t6 switched off
    elif kernel == T7:
        assert wide.kernel == T7 and narrow.kernel == T6   # (narrow bands stay with the one-wave kernel)
    else:
        assert wide.kernel == kernel and narrow.kernel == kernel
    assert wide.def_pen == narrow.def_pen == (0 if "generic" in value or kernel == LDS else 1)
    if value in ("128", "256", "512"):
        assert wide.nt == int(value) and narrow.fam_nt == int(value)
    if kernel == T7:
        assert wide.nt == 256 and wide.hg_cols == 4096 and wide.win_mask == 4095   # an ordinary launch: 256 threads
    for s in (wide, narrow):
        assert s.nt in INSTANTIATED[s.kernel] and s.lds <= LDS_LIMIT


def test_shape_switches(lib, monkeypatch):
    monkeypatch.setenv("VGA_POA_NT", "512")
    assert shape(lib).nt == 512 and shape(lib, arena=False).nt == 512
    monkeypatch.setenv("VGA_POA_NT", "1024")
    assert shape(lib).nt == 1024
    monkeypatch.setenv("VGA_POA_NT", "200")   # not a multiple of 64
    assert shape(lib).nt == 512
    monkeypatch.delenv("VGA_POA_NT")
    monkeypatch.setenv("VGA_POA_WINDOW", "256")
    s = shape(lib)
    assert s.kernel == T5 and s.hg_cols == 256 and s.win_mask == 255
    monkeypatch.setenv("VGA_POA_WINDOW", "0")   # every column
    assert shape(lib).win_mask == 0xFFFFFFFF
    monkeypatch.delenv("VGA_POA_WINDOW")
    monkeypatch.setenv("VGA_POA_KERNEL", "t7")
    monkeypatch.setenv("VGA_POA_T7_NT", "128")
    monkeypatch.setenv("VGA_POA_T7_WINDOW", "1024")
    s = shape(lib)
    assert s.kernel == T7 and s.nt == 128 and s.hg_cols == 1024 and s.win_mask == 1023 and s.lds == lib.t_t5_bytes(1024, s.lds_cols, 128)
    monkeypatch.delenv("VGA_POA_T7_WINDOW")
    monkeypatch.setenv("VGA_POA_T7_NT", "1024")
    s = shape(lib)
    assert s.kernel == T7 and s.nt == 1024 and s.hg_cols == 8192   # (the power of two that holds 1.6 x the widest estimate)


def test_call_level_switches_keep_their_meaning(lib, monkeypatch):
    cap = C.c_ulonglong()
    assert lib.t_tb_fused() == 1 and lib.t_arenas(C.byref(cap)) == 0 and cap.value == 0
    monkeypatch.setenv("VGA_POA_TB", "wave")
    assert lib.t_tb_fused() == 0
    monkeypatch.setenv("VGA_POA_TB", "fused")
    assert lib.t_tb_fused() == 1
    monkeypatch.setenv("VGA_POA_ARENAS", "0")
    assert lib.t_arenas(C.byref(cap)) == 1
    monkeypatch.setenv("VGA_POA_ARENAS", "24")
    assert lib.t_arenas(C.byref(cap)) == 0 and cap.value == 24


def test_230_kbp_query_with_the_long_problem_shape_pinned(lib, monkeypatch):
    """test_poa_230_kbp_query_with_the_long_problem_launch_shape, without the GPU: beyond ~228 kbp the query's column codes leave
    no room for an 8 192-column window beside 1 024 threads' headers"""
    monkeypatch.setenv("VGA_POA_WINDOW", "8192")
    monkeypatch.setenv("VGA_POA_NT", "1024")
    s = shape(lib, max_q=200000, mean_w=200000.0, max_w=200001.0, left=2, arena=False)
    assert s.kernel == T5 and s.nt == 1024 and s.hg_cols == 8192
    for q in (229000, 230000, 250000, 279000):
        s = shape(lib, max_q=q, mean_w=float(q), max_w=q + 1.0, left=2, arena=False)
        assert s.kernel == T5 and s.hg_cols < 8192 and _window_is_sane(s) and s.hg_cols >= 512
        assert s.nt in INSTANTIATED[T5] and s.lds <= LDS_LIMIT
    s = shape(lib, max_q=230000, mean_w=230000.0, max_w=230001.0, left=2, arena=False)
    assert s.hg_cols == 4096 and s.nt == 1024   # halved once; the workgroup stays


def test_every_shape_fits_or_is_the_smallest(lib):
    rng = random.Random(20261016)
    gap_sets = [DEFAULT, (5, 2, 24, 1), (31, 33, 24, 1), (6, 3, 200, 1), (4, 0, 24, 1), (10, 6, 24, 1), (32, 2, 24, 1)]
    seen = set()
    for _ in range(20000):
        gaps = rng.choice(gap_sets)
        fam = lib.t_family(_gaps(gaps))
        q = int(10 ** rng.uniform(1.0, 5.45))
        if lib.t_min_lds(fam, q) > LDS_LIMIT:
            continue   # not admitted
        mean_w = rng.uniform(10.0, min(q + 1.0, 30000.0))
        max_w = mean_w * rng.uniform(1.0, 3.0)
        arena = fam == T5 and rng.random() < 0.7
        s = shape(lib, max_q=q, mean_w=mean_w, max_w=max_w, left=rng.choice((1, 7, 300, 2048, 100000)), in_flight=rng.choice((0, 2048, 4096)),
                  n_cu=rng.choice((64, 256)), giant=rng.random() < 0.15, general=rng.random() < 0.2, arena=arena,
                  fused=fam != LDS and rng.random() < 0.8, gaps=gaps)
        seen.add(s.kernel)
        assert s.kernel in ((LDS,), (T4,), (T5, T6, T7))[fam], (gaps, s.kernel)
        assert s.nt in INSTANTIATED[s.kernel], (s.kernel, s.nt)
        assert s.lds_cols == lib.t_lds_cols(q) and _window_is_sane(s)
        smallest = s.nt == min(INSTANTIATED[s.kernel]) and (s.kernel in (LDS, T6) or s.hg_cols <= (1024 if s.kernel == T7 else 512))
        assert s.lds <= LDS_LIMIT or smallest, (gaps, q, s.kernel, s.nt, s.hg_cols, s.lds)
    assert seen == {LDS, T4, T5, T6, T7}
