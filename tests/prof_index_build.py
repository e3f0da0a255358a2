"""diagnostic: Index::build on the host vs vga_index_build_kmers on the GPU (config-5 generator, seed 77, 1 and 8 Mbp,
k = 11 and 15).  Per case: wall time of HostIndex.build_from_gfa without / with ctx (both ending in a device synchronise),
the per-kernel times of the device build, the vga_index_upload time the device-built probe tables save, and whether the
arrays are equal.  One JSON line per case on stdout.

    python tests/prof_index_build.py [--sizes 1000000,8000000] [--ks 11,15] [--tmp DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

p = ge.load_package()


def same(a, b):
    if a["kmer_keys"] != b["kmer_keys"] or not np.array_equal(a["kmer_starts"], b["kmer_starts"]):
        return False
    x, y = a["kmer_pos_table"], b["kmer_pos_table"]
    return len(x) == len(y) and all(np.array_equal(x[n], y[n]) for n in x.dtype.names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,8000000")
    ap.add_argument("--ks", default="11,15")
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    tmp = a.tmp or tempfile.mkdtemp(prefix="prof_index_")
    ctx = p.Context(0)
    for size in [int(x) for x in a.sizes.split(",")]:
        gfa = os.path.join(tmp, f"syn{size}.gfa")
        if not os.path.exists(gfa):
            p.readsim.synth_pangenome(gfa, size, seed=77)
        for k in [int(x) for x in a.ks.split(",")]:
            p.HostIndex.build_from_gfa(gfa, k, ctx=ctx)  # warm-up: module load, first allocations
            t0 = time.perf_counter()
            host = p.HostIndex.build_from_gfa(gfa, k)
            ctx.synchronize()
            t_host = time.perf_counter() - t0
            t0 = time.perf_counter()
            dev = p.HostIndex.build_from_gfa(gfa, k, ctx=ctx)
            ctx.synchronize()
            t_dev = time.perf_counter() - t0
            kt = ctx.kernel_times()
            up = p.Context(0)
            t0 = time.perf_counter()
            host.upload(up)
            up.synchronize()
            t_upload = time.perf_counter() - t0
            up.close()
            ha, da = host.arrays(), dev.arrays()
            print(json.dumps({"bp": size, "k": k, "n_kmers": len(ha["kmer_starts"]), "n_kmer_pos": len(ha["kmer_pos_table"]),
                              "host_build_s": round(t_host, 3), "gpu_build_s": round(t_dev, 3),
                              "kernels_ms": {t["name"]: round(t["ms"], 3) for t in kt},
                              "upload_of_host_index_s": round(t_upload, 3), "equal": same(ha, da)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
