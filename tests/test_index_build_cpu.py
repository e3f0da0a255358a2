"""CPU-side checks of the GPU index build (vga_index_build_kmers): the library exports it, the bindings and the CLI
expose it, and without a GPU it refuses (VGA_ERR_NO_DEVICE) instead of falling back to the host builder."""
import ctypes as C
import os
import subprocess

import pytest

from helpers import DATA, ROOT, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")


def _has_gpu():
    L = pkg().load_library()
    h = C.c_void_p()
    if L.vga_ctx_create(0, C.byref(h)) == 0:
        L.vga_ctx_destroy(h)
        return True
    return False


def test_library_exports_the_index_build():
    L = pkg().load_library()
    for sym in ("vga_index_build_kmers", "vga_index_kmers_free"):
        assert hasattr(L, sym), sym
    assert L.vga_abi_version() == 6


def test_bindings_expose_the_index_build():
    p = pkg()
    assert {"vga_index_build_kmers", "vga_index_kmers_free"} <= set(p.binding.ABI_SYMBOLS)
    for name in ("index_build_kmers",):
        assert callable(getattr(p.binding.Context, name))
    for name in ("graph_desc", "kmer_arrays", "index_kmers_free"):
        assert callable(getattr(p.binding, name))
    import inspect

    assert "ctx" in inspect.signature(p.HostIndex.build_from_gfa).parameters
    hl = p.hostlib.load_library()
    assert hasattr(hl, "vgh_index_build_from_gfa_on_device")


def test_kmers_free_zeroes_an_empty_desc():
    b = pkg().binding
    a = pkg().HostIndex.build_from_gfa(DRB1, 11).arrays()
    d = b.graph_desc(11, a["seq_fwd"], a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])
    b.index_kmers_free(d)
    assert (d.n_kmers, d.n_kmer_pos) == (0, 0) and not d.kmer_keys


def test_no_device_no_fallback(tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is visible: the refusal path is not reachable")
    p = pkg()
    b = p.binding
    L = p.load_library()
    a = p.HostIndex.build_from_gfa(DRB1, 11).arrays()
    d = b.graph_desc(11, a["seq_fwd"], a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])
    assert L.vga_index_build_kmers(None, C.byref(d), 100, 100) == -6  # VGA_ERR_NO_DEVICE
    assert d.n_kmers == 0 and not d.kmer_pos_table
    hl = p.hostlib.load_library()
    assert not hl.vgh_index_build_from_gfa_on_device(DRB1.encode(), 11, 100, 100, None)
    assert "VGA_ERR_NO_DEVICE" in hl.vgh_last_error().decode()


def test_cli_index_device_without_gpu_writes_nothing(tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is visible: the refusal path is not reachable")
    pkg()
    exe = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
    r = subprocess.run([exe, "index", "-i", DRB1, "-k", "11", "-o", str(tmp_path / "x"), "--device", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "VGA_ERR_NO_DEVICE" in r.stderr and "no CPU path" in r.stderr
    assert not os.path.exists(tmp_path / "x.idx")
    u = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert "--device N" in u.stderr


def test_host_index_files_are_deterministic(tmp_path):
    """the .idx bytes of one graph do not depend on the run (vga_kmerpos padding is written as zeros)"""
    pkg()
    exe = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
    for name in ("a", "b"):
        subprocess.run([exe, "index", "-i", DRB1, "-k", "11", "-o", str(tmp_path / name)], check=True, capture_output=True, timeout=300)
    assert (tmp_path / "a.idx").read_bytes() == (tmp_path / "b.idx").read_bytes()
