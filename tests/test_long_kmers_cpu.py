"""k-mers of 16 to 32 bases, the parts that need no GPU: the host builder's index at long k against the oracle's, the shared
header of the hashed probe table (rs-vgaligner_amd/csrc/vga_probe_hash.hpp) compiled for the host, the register and scratch
budget of K1's four instantiations from a cross-compile for gfx950, and the limit the header and the binding publish."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
TEST_GFA = os.path.join(DATA, "test.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


# ---- the host builder at long k (the half of the route `vgaligner index -k 19` + `vgaligner map` relies on)
def _same_index(a, b, what):
    assert set(a) == set(b), what
    for f in a:
        x, y = a[f], b[f]
        if isinstance(x, np.ndarray) and x.dtype.names:
            assert len(x) == len(y), (what, f, len(x), len(y))
            for n in x.dtype.names:
                assert np.array_equal(x[n], y[n]), (what, f, n)
        elif isinstance(x, (bytes, int)):
            assert x == y, (what, f)
        else:
            assert np.array_equal(np.asarray(x, np.uint64), np.asarray(y, np.uint64)), (what, f)


@pytest.mark.parametrize("k", [19, 32])
@pytest.mark.parametrize("gfa", [DRB1, TEST_GFA], ids=["drb1", "test_gfa"])
def test_host_index_equals_oracle_and_survives_the_idx_file(oracle, tmp_path, gfa, k):
    p = pkg()
    want = oracle_index_arrays(oracle.Index(oracle.Graph.from_gfa(gfa), k))
    hi = p.HostIndex.build_from_gfa(gfa, k)
    got = hi.arrays()
    assert got["k"] == k and len(got["kmer_keys"]) == k * len(got["kmer_starts"]) > 0
    _same_index(got, want, "host builder")
    path = str(tmp_path / "long.idx")
    hi.store(path)
    _same_index(p.HostIndex.load(path).arrays(), want, ".idx round trip")


# ---- the shared header, compiled for the host
HARNESS = r"""
#include "vga_probe_hash.hpp"
#include <vector>
static_assert(sizeof(vga_hash_slot) == 16 && alignof(vga_hash_slot) == 16, "one 16-byte load per slot");
extern "C" {
unsigned long long t_capacity(unsigned long long n) { return vga_hash_capacity(n); }
unsigned long long t_mix(unsigned long long x) { return vga_hash_mix64(x); }
unsigned t_first(unsigned long long key, unsigned mask) { return vga_hash_first_slot(key, mask); }
unsigned t_next(unsigned slot, unsigned mask) { return vga_hash_next_slot(slot, mask); }
void *t_new(unsigned long long cap) {
    auto *v = new std::vector<vga_hash_slot>(cap);
    for (auto &s : *v) { s.key = ~0ull; s.hdr_all = VGA_HASH_EMPTY; s.hdr_ff = VGA_HASH_EMPTY; }  // the upload's memset 0xFF
    return v;
}
void t_free(void *t) { delete (std::vector<vga_hash_slot> *)t; }
// key i gets the header pair (i, n + i); returns how many found a slot
unsigned long long t_insert(void *t, const unsigned long long *keys, unsigned long long n) {
    auto &v = *(std::vector<vga_hash_slot> *)t;
    unsigned long long ok = 0;
    for (unsigned long long i = 0; i < n; i++) ok += vga_hash_insert_host(v.data(), (uint32_t)(v.size() - 1), keys[i], (uint32_t)i, (uint32_t)(n + i));
    return ok;
}
// out[i]: the hdr_all of key i, or VGA_HASH_EMPTY when absent; returns how many were found with a consistent hdr_ff
unsigned long long t_find(void *t, const unsigned long long *keys, unsigned long long n, unsigned long long n_ins, unsigned *out) {
    auto &v = *(std::vector<vga_hash_slot> *)t;
    unsigned long long ok = 0;
    for (unsigned long long i = 0; i < n; i++) {
        const vga_hash_slot *s = vga_hash_find_host(v.data(), (uint32_t)(v.size() - 1), keys[i]);
        out[i] = s ? s->hdr_all : VGA_HASH_EMPTY;
        if (s && s->key == keys[i] && s->hdr_ff == s->hdr_all + n_ins) ok++;
    }
    return ok;
}
}
"""


@pytest.fixture(scope="module")
def hashlib_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("probe_hash")
    src, so = d / "harness.cpp", d / "harness.so"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    for name, res, args in (("t_capacity", u64, [u64]), ("t_mix", u64, [u64]), ("t_first", u32, [u64, u32]), ("t_next", u32, [u32, u32]),
                            ("t_new", vp, [u64]), ("t_free", None, [vp]), ("t_insert", u64, [vp, C.POINTER(u64), u64]),
                            ("t_find", u64, [vp, C.POINTER(u64), u64, u64, C.POINTER(u32)])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def test_capacity_rule_and_slot_arithmetic(hashlib_host):
    L = hashlib_host
    for n in [0, 1, 7, 8, 9, 1000, 4096, 4097, 248984, 1481234, (1 << 20), (1 << 20) + 1, 1 << 30]:
        cap = L.t_capacity(n)
        assert cap >= 2 * n and cap >= 16 and cap & (cap - 1) == 0, (n, cap)
        assert cap < 4 * max(n, 8) or n < 8, (n, cap)  # (the smallest such power of two)
        assert cap <= 1 << 31
    assert L.t_capacity((1 << 30) + 1) == 0  # header indices and slot numbers are 32 bits
    # the murmur3 finaliser: fixed points and a published vector of the bijection
    assert L.t_mix(0) == 0 and L.t_mix(1) == 0xB456BCFC34C2CB2C
    mask = (1 << 12) - 1
    assert L.t_first(0x0123456789ABCDEF, mask) == L.t_mix(0x0123456789ABCDEF) & mask
    assert L.t_next(mask, mask) == 0 and L.t_next(5, mask) == 6


def _pack(keys_bytes, k):
    """2-bit packed k-mers (A=0 C=1 G=2 T=3, first base highest), as vga_index_upload packs them"""
    a = np.frombuffer(keys_bytes, dtype=np.uint8).reshape(-1, k)
    code = np.full(256, 255, np.uint8)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    c2 = code[a]
    assert int(c2.max()) <= 3
    out = np.zeros(len(a), np.uint64)
    for t in range(k):
        out = (out << np.uint64(2)) | c2[:, t].astype(np.uint64)
    return out


def test_drb1_k32_insert_and_lookup_on_the_host(hashlib_host):
    L = hashlib_host
    arr = pkg().HostIndex.build_from_gfa(DRB1, 32).arrays()
    keys = np.ascontiguousarray(_pack(arr["kmer_keys"], 32))
    n = len(keys)
    assert n > 1_400_000 and len(np.unique(keys)) == n
    cap = L.t_capacity(n)
    t = L.t_new(cap)
    try:
        kp = keys.ctypes.data_as(C.POINTER(C.c_uint64))
        assert L.t_insert(t, kp, n) == n
        out = np.zeros(n, np.uint32)
        assert L.t_find(t, kp, n, n, out.ctypes.data_as(C.POINTER(C.c_uint32))) == n
        assert np.array_equal(out, np.arange(n, dtype=np.uint32))
        # 1 000 absent keys, among them 0 (poly-A) and ~0 (poly-T, the key bits of an empty slot)
        rng = np.random.default_rng(32)
        absent = np.concatenate([np.array([0, 0xFFFFFFFFFFFFFFFF], np.uint64), rng.integers(0, 1 << 63, 1200, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                                 keys[:200] ^ np.uint64(1)])
        absent = np.ascontiguousarray(absent[~np.isin(absent, keys)][:1000])
        assert len(absent) == 1000 and absent[0] == 0 and absent[1] == 0xFFFFFFFFFFFFFFFF
        out = np.zeros(1000, np.uint32)
        assert L.t_find(t, absent.ctypes.data_as(C.POINTER(C.c_uint64)), 1000, n, out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
        assert (out == 0xFFFFFFFF).all()
    finally:
        L.t_free(t)


# ---- K1's instantiations, cross-compiled
@pytest.fixture(scope="module")
def k1_isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("k1isa")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--save-temps", "-c",
                           os.path.join(CSRC, "vga_map.hip"), "-o", str(d / "vga_map.o")], cwd=str(d), stderr=subprocess.DEVNULL)
    s = [f for f in os.listdir(d) if f.endswith(".s") and "gfx950" in f]
    assert len(s) == 1, os.listdir(d)
    return open(d / s[0]).read()


def _kernel_entries(text, stem):
    """{mangled name: its metadata entry} of the kernels whose name starts with _Z<len><stem>"""
    out = {}
    for m in re.finditer(r"\.name:\s+(_Z\d+" + stem + r"\w*)\n", text):
        a = text.rfind("\n  - ", 0, m.start())
        b = text.find("\n  - ", m.end())
        out[m.group(1)] = text[a:b if b >= 0 else len(text)]
    return out


def test_k1_variants_exist_without_scratch(k1_isa):
    entries = _kernel_entries(k1_isa, "k_kmer_probe")
    # template arguments <EMIT, HASH>: Lb0 / Lb1
    want = {"ILb0ELb0E": "count, 32-bit key", "ILb1ELb0E": "emit, 32-bit key", "ILb0ELb1E": "count, 64-bit key", "ILb1ELb1E": "emit, 64-bit key"}
    for tag, what in want.items():
        names = [n for n in entries if "k_kmer_probe" + tag in n]
        assert len(names) == 1, (what, sorted(entries))
        e = entries[names[0]]
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", e).group(1))
        print(what, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
        assert field("private_segment_fixed_size") == 0, what
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, what
        assert field("group_segment_fixed_size") <= 320, what  # codes[256 + 32] + the scan's 4 words
    assert len(entries) == 4, sorted(entries)

def test_insert_kernel_without_scratch(tmp_path):
    out = str(tmp_path / "ctx.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_ctx.hip"), "-o", out], stderr=subprocess.DEVNULL)
    entries = _kernel_entries(open(out).read(), "k_probe_hash_insert")
    assert len(entries) == 1, sorted(entries)
    e = next(iter(entries.values()))
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", e).group(1)) == 0


# ---- the published limit
def test_max_kmer_length_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    m = re.search(r"^#define\s+VGA_MAX_KMER_LENGTH\s+(\d+)\s*$", header, flags=re.M)
    assert m and int(m.group(1)) == 32 == pkg().binding.VGA_MAX_KMER_LENGTH
