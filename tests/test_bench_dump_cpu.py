"""bench.py --dump-outputs on CPU: the arrays it writes from a step's vga_map_result / vga_align_result (here C structs
filled by hand) are float32 / float64, stay within the size bound, come out the same twice, and the concatenated
sample splits back into each sampled read's own results with the per-read counts."""
import ctypes as C
import os

import numpy as np

from helpers import ROOT, pkg  # noqa: F401  (ROOT on sys.path: bench.py is importable)


def fake_results(n_reads, seed=3):
    """A vga_map_result and a vga_align_result of n_reads reads with random contents; the numpy buffers stay alive in `keep`."""
    b = pkg().binding
    rng = np.random.default_rng(seed)
    keep = []

    def buf(a, ctype):
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ctype))

    def offsets(counts):
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)

    na = rng.integers(0, 40, n_reads)
    nc = rng.integers(0, 4, n_reads)
    a_off, c_off = offsets(na), offsets(nc)
    n_a, n_c = int(a_off[-1]), int(c_off[-1])
    cn = rng.integers(1, 6, n_c)
    ca_off = offsets(cn)
    q = b.MapResult()
    q.n_reads, q.n_anchors, q.n_chains = n_reads, n_a, n_c
    q.anchor_off = buf(a_off, C.c_uint64)
    q.query_begin = buf(rng.integers(0, 10000, n_a).astype(np.uint32), C.c_uint32)
    q.target_begin = buf(rng.integers(0, 1 << 32, n_a, dtype=np.uint64).astype(np.uint32), C.c_uint32)
    q.target_end = buf(rng.integers(0, 1 << 32, n_a, dtype=np.uint64).astype(np.uint32), C.c_uint32)
    q.curr_max = buf(rng.random(n_reads) * 1000, C.c_double)
    q.chain_off = buf(c_off, C.c_uint64)
    q.chain_placeholder = buf(rng.integers(0, 2, n_c).astype(np.uint8), C.c_uint8)
    q.chain_anchor_off = buf(ca_off, C.c_uint64)
    q.chain_anchor_idx = buf(rng.integers(0, 40, int(ca_off[-1])).astype(np.uint32), C.c_uint32)

    def text(counts):
        off = offsets(counts + 1)  # every string carries its NUL
        t = rng.integers(ord("0"), ord("z"), int(off[-1])).astype(np.uint8)
        t[off[1:].astype(np.int64) - 1] = 0
        return off, t

    r = b.AlignResult()
    r.n_reads = n_reads
    r.aligned = buf(rng.integers(0, 2, n_reads).astype(np.uint8), C.c_uint8)
    p_off = offsets(rng.integers(0, 30, n_reads))
    r.path_off = buf(p_off, C.c_uint64)
    r.path_handles = buf(rng.integers(0, 1 << 40, int(p_off[-1])).astype(np.uint64), C.c_uint64)
    for f in ("path_length", "path_start", "path_end", "block_length"):
        setattr(r, f, buf(rng.integers(0, 1 << 31, n_reads).astype(np.uint32), C.c_uint32))
    r.best_score = buf(rng.integers(-50000, 50000, n_reads).astype(np.int32), C.c_int32)
    g_off, g = text(rng.integers(0, 200, n_reads))
    s_off, s = text(rng.integers(0, 500, n_reads))
    r.cigar_off, r.cigar = buf(g_off, C.c_uint64), buf(g, C.c_char)
    r.cs_off, r.cs = buf(s_off, C.c_uint64), buf(s, C.c_char)
    return q, r, keep, dict(a_off=a_off, c_off=c_off, ca_off=ca_off, p_off=p_off, g_off=g_off, s_off=s_off, g=g, s=s)


def test_dump_outputs_are_bounded_deterministic_and_split_per_read(tmp_path):
    import bench

    q, r, keep, raw = fake_results(3000)
    got = bench.capture_outputs(q, r)
    assert all(np.array_equal(v, got[k]) for k, v in bench.capture_outputs(q, r).items())
    bench.write_outputs(str(tmp_path), got)
    files = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))}
    assert set(files) == set(got)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))) <= 64 * 1000 * 1000
    assert files["read_index"].tolist() == list(range(3000))
    best = np.ctypeslib.as_array(r.best_score, shape=(3000,))
    assert files["best_score"].tolist() == best.tolist()
    assert files["n_anchors"].tolist() == np.diff(raw["a_off"].astype(np.int64)).tolist()

    sample = files["sample_reads"].astype(np.int64)
    assert len(sample) == bench.DUMP_SAMPLE_READS and np.all(np.diff(sample) > 0)
    tb_all = np.ctypeslib.as_array(q.target_begin, shape=(int(q.n_anchors),))
    pos = {"a": 0, "g": 0, "c": 0}
    for i in sample:
        a0, a1 = int(raw["a_off"][i]), int(raw["a_off"][i + 1])
        n = int(files["n_anchors"][i])
        assert files["sample_anchor_target_begin"][pos["a"]:pos["a"] + n].tolist() == tb_all[a0:a1].tolist()
        pos["a"] += n
        g0, g1 = int(raw["g_off"][i]), int(raw["g_off"][i + 1]) - 1
        n = int(files["cigar_len"][i])
        assert n == g1 - g0
        assert files["sample_cigar"][pos["g"]:pos["g"] + n].tolist() == raw["g"][g0:g1].tolist()
        pos["g"] += n
        pos["c"] += int(files["n_chains"][i])
    assert pos["a"] == len(files["sample_anchor_query_begin"]) and pos["g"] == len(files["sample_cigar"])
    assert pos["c"] == len(files["sample_chain_n_anchors"]) == len(files["sample_chain_placeholder"])
    assert int(files["sample_chain_n_anchors"].sum()) == len(files["sample_chain_anchor_idx"])


def test_dump_outputs_sample_shrinks_to_the_size_bound(monkeypatch):
    import bench

    q, r, keep, raw = fake_results(500)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 300 * 1000)
    monkeypatch.setattr(bench, "DUMP_PER_READ_MAX", 256)
    got = bench.capture_outputs(q, r)
    assert len(got["read_index"]) == 256 and np.all(np.diff(got["read_index"]) > 0)
    assert 0 < len(got["sample_reads"]) < bench.DUMP_SAMPLE_READS
    total = sum(a.size * (4 if k in ("sample_cigar", "sample_cs") else 8) for k, a in got.items())
    assert total <= 300 * 1000
    q.n_reads = 0
    empty = bench.capture_outputs(q, None)
    assert all(a.size == 0 for a in empty.values())
