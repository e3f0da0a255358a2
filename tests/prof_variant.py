"""diagnostic: what the variant call costs, and what it saves.  One JSON object on stdout
(profiles/variant_calls.json).  Every measurement runs in a child process of its own with a time limit of its own, and the sides of
a comparison alternate, so that both see the same box in the same minutes; the first child that fails ends the script.
`--parent-lib` names a libvga_hip.so built from the parent commit by the same compiler (the binding's VGA_LIB).

  bench_ab   the switch off costs nothing: `python bench.py --gpus 1 --steps 3 --warmup 1` (config 3) with this tree's library and
             with the parent's, alternating, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  seam       the three kernels alone through vga_variant_call_table on a table of 22 595 rows (DRB1's bases) and of 1 000 000
             (config 5's): depth 30 of the base's own letter, one base in 200 with a second allele; the kernel times from
             vga_last_kernel_times, the wall time of the call (which uploads 57 bytes per row first) and the calls that came back.
  routes     `vgaligner map --also-align` on `--route-reads` reads of 3 kbp with --pileup alone and with --call-variants alone,
             alternating, VGA_TRACE=1: the time to fetch the whole table (vga_pileup_read) and to write <out>-pileup.tsv against
             the time of the call (vga_variant_call) and of <out>-variants.tsv, and the size of either file; config 3 and config 5.

    python tests/prof_variant.py --parent-lib PATH [--parts bench_ab,seam,routes] [--repeats 3] [--route-reads 200]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRB1 = os.path.join(ROOT, "tests", "golden", "data", "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
VC = ("k_vc_count", "k_vc_scan", "k_vc_emit")


def child_seam(n, repeats):
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    ctx = p.Context(0)
    rng = np.random.default_rng(20)
    own = rng.integers(0, 4, size=n)
    tab = np.zeros((n, 7), dtype=np.uint64)
    tab[np.arange(n), own] = 30
    alt = np.flatnonzero(rng.random(n) < 0.005)
    tab[alt, own[alt]] = 15
    tab[alt, (own[alt] + 1) % 4] = 15
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[own].tobytes()
    ctx.variant_call_table(tab[:1000], letters[:1000])  # (warm-up)
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = ctx.variant_call_table(tab, letters, cap=len(alt) + 16)
        wall = time.perf_counter() - t0
        k = {t["name"]: t for t in ctx.kernel_times()}
        runs.append({"call_wall_ms": round(wall * 1e3, 3), **{name + "_ms": round(k[name]["ms"], 4) for name in VC if name in k}})
    assert out["n_calls"] == len(alt)
    best = min(r["k_vc_count_ms"] for r in runs)
    print(json.dumps({"rows": n, "bytes_read_per_row": 57, "n_tested": out["n_tested"], "n_calls": out["n_calls"], "runs": runs,
                      "k_vc_count_best_ms": best, "k_vc_count_best_GB_per_s": round(n * 57 / (best * 1e-3) / 1e9, 1)}))
    ctx.close()


def run_child(args, env=None, limit=600, exe=None):
    pr = subprocess.run(([sys.executable] if exe is None else [exe]) + args, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    if pr.returncode != 0:
        sys.stderr.write(pr.stdout[-2000:] + pr.stderr[-4000:])
        raise SystemExit("child failed (%d): %s" % (pr.returncode, " ".join(args)))
    print("done:", " ".join(args)[-100:], file=sys.stderr, flush=True)
    return pr


def last_json(pr):
    return json.loads([l for l in pr.stdout.splitlines() if l.startswith("{")][-1])


def routes(workload, n_reads, repeats):
    import __graft_entry__ as ge

    p = ge.load_package()
    d = tempfile.mkdtemp(prefix="vga_prof_variant_")
    gfa = DRB1
    if workload == "config5":
        gfa = os.path.join(d, "config5.gfa")
        p.readsim.synth_pangenome(gfa)
    reads = p.readsim.simulate_reads(gfa, n_reads, 3000, 0.03, 0.03, 0.04, seed=77)
    fa = os.path.join(d, "r.fa")
    p.readsim.write_fasta(reads, fa)
    run_child(["index", "-i", gfa, "-k", "11", "-o", os.path.join(d, "g")], exe=EXE, limit=900)
    common = ["map", "-i", os.path.join(d, "g"), "-f", fa, "-p", "abpoa", "--also-align", "-G", gfa]
    env = dict(os.environ, VGA_TRACE="1")
    mark = lambda text, what: float(re.search(re.escape(what) + r"\s+\+\s*([0-9.]+) ms", text).group(1))
    row = {"workload": workload, "reads": n_reads, "table": [], "call": []}
    for _ in range(repeats):
        for side, switch in (("table", "--pileup"), ("call", "--call-variants")):
            pre = os.path.join(d, side)
            err = run_child(common + ["-o", pre, switch], exe=EXE, env=env, limit=900).stderr
            took = re.search(r"pileup table read in ([0-9.]+) ms, variants called in ([0-9.]+) ms", err)
            if side == "table":
                row["table"].append({"vga_pileup_read_ms": float(took.group(1)), "sum_and_write_tsv_ms": mark(err, "pileup table written"),
                                     "tsv_bytes": os.path.getsize(pre + "-pileup.tsv")})
            else:
                row["call"].append({"vga_variant_call_ms": float(took.group(2)), "write_tsv_ms": mark(err, "variants written"),
                                    "tsv_bytes": os.path.getsize(pre + "-variants.tsv"),
                                    "stderr": re.search(r"call-variants: .*", err).group(0)})
    row["graph_bases"] = sum(1 for _ in open(os.path.join(d, "table-pileup.tsv"))) - 1
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parts", default="bench_ab,seam,routes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--route-reads", type=int, default=200)
    ap.add_argument("--workloads", default="config3,config5")
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child:
        child_seam(int(a.child[1]), int(a.child[2]))
        return
    me = os.path.abspath(__file__)
    out = {"what": "what the variant call costs and saves on one MI355X (DESIGN.md section 20); no figure here is asserted by a test"}
    parts = a.parts.split(",")
    if "seam" in parts:
        out["seam"] = [last_json(run_child([me, "--child", "seam", str(n), "5"])) for n in (22595, 1000000)]
    if "routes" in parts:
        out["routes"] = [routes(wl, a.route_reads, a.repeats) for wl in a.workloads.split(",")]
    if "bench_ab" in parts:
        assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: a libvga_hip.so built from the parent commit"
        runs = {"branch": [], "parent": []}
        for _ in range(a.repeats):
            for side in ("branch", "parent"):
                env = dict(os.environ)
                if side == "parent":
                    env["VGA_LIB"] = os.path.abspath(a.parent_lib)
                else:
                    env.pop("VGA_LIB", None)
                runs[side].append(last_json(run_child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env))["value"])
        rng = {s: [min(v), max(v)] for s, v in runs.items()}
        out["bench_ab"] = {"bench": "python bench.py --gpus 1 --steps 3 --warmup 1", "metric": "aligned reads/s, config 3",
                           "order": "branch and parent alternating, processes of their own, one box; the parent's library built from the parent commit with the same compiler (VGA_LIB)",
                           "runs": runs, "branch_range": rng["branch"], "parent_range": rng["parent"],
                           "ranges_overlap": rng["branch"][0] <= rng["parent"][1] and rng["parent"][0] <= rng["branch"][1]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
