"""diagnostic: what counting read coverage costs.  One JSON object on stdout (profiles/coverage.json).
Every measurement runs in a child process of its own, and the processes of a pair alternate, so that both sides of a comparison
see the same box in the same minutes.  `--parent-lib` names a libvga_hip.so built from the parent commit (the binding's VGA_LIB).

  bench_ab   counting off costs nothing: `python bench.py` (config 3) with this tree's library and with the parent's,
             alternating, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  step       counting on is cheap: config 3 and config 5 steps (10 000 x 10 kbp reads, seed 77: map + align, the step bench.py
             times) with the parent's library, with this one counting off, and with this one counting on, alternating; aligned
             reads/s and, from vga_last_kernel_times, the busy time per step of k_cov_runs, k_cov_add and poa_text (k_poa_text).
  cli        what --coverage-only saves: wall clock of `vgaligner map` on `--cli-reads` config 5 reads with --also-align, with
             --coverage and with --coverage-only, and the bytes each wrote.

    python tests/prof_coverage.py --parent-lib PATH [--parts bench_ab,step,cli] [--repeats 4] [--reads 10000] [--steps 3] [--cli-reads 100000]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRB1 = os.path.join(ROOT, "tests", "golden", "data", "DRB1-3123.gfa")
BUSY = ("k_cov_runs", "k_cov_add", "poa_text", "poa_band_dp")


def child_step(gfa, n_reads, steps, warmup, coverage):
    """one process: reads/s of the timed steps and the kernels' busy time per step"""
    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(gfa, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(gfa, n_reads)])
    if coverage:
        ctx.coverage_begin()
    for _ in range(warmup):
        b.map_align_raw()
    ctx.synchronize()
    busy = {n: 0.0 for n in BUSY}
    aligned = 0
    t0 = time.perf_counter()
    for _ in range(steps):
        st = b.map_align_raw()
        aligned += st["aligned"]
        for k in st["kernels"]:
            if k["name"] in busy:
                busy[k["name"]] += k["busy_ms"]
    ctx.synchronize()
    dt = time.perf_counter() - t0
    out = {"aligned_reads_per_s": round(aligned / dt, 1), "ms_per_step": round(dt / steps * 1e3, 1),
           "busy_ms_per_step": {n: round(v / steps, 3) for n, v in busy.items()}}
    if coverage:
        base, node, edge, n_al = ctx.coverage()
        out["counted"] = {"alignments": n_al, "covered_bases": int(base.sum(dtype="uint64")), "node_visits": int(node.sum(dtype="uint64")),
                          "edge_visits": int(edge.sum(dtype="uint64"))}
    print(json.dumps(out), flush=True)


def run_json(cmd, env=None, timeout=3000):
    pr = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    if pr.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (" ".join(cmd), pr.returncode, pr.stderr[-600:]))
    return json.loads(pr.stdout.strip().splitlines()[-1])


def lib_env(parent_lib):
    env = dict(os.environ)
    env.pop("VGA_LIB", None)
    if parent_lib:
        env["VGA_LIB"] = parent_lib
    return env


def bench_ab(parent_lib, repeats):
    vals = {"branch": [], "parent": []}
    for rep in range(repeats):
        for side in (("branch", "parent") if rep % 2 == 0 else ("parent", "branch")):
            line = run_json([sys.executable, os.path.join(ROOT, "bench.py")], env=lib_env(parent_lib if side == "parent" else None))
            vals[side].append(line["value"])
            print(side, line["value"], file=sys.stderr, flush=True)
    lo_b, hi_b, lo_p, hi_p = min(vals["branch"]), max(vals["branch"]), min(vals["parent"]), max(vals["parent"])
    return {"command": "python bench.py", "metric": "aligned reads/s, config 3", "runs": vals, "branch_range": [lo_b, hi_b], "parent_range": [lo_p, hi_p],
            "ranges_overlap": bool(lo_b <= hi_p and lo_p <= hi_b), "branch_best_below_parent_worst": bool(hi_b < lo_p)}


def step(parent_lib, gfa, n_reads, steps, warmup, repeats):
    sides = {"parent": (parent_lib, 0), "branch_off": (None, 0), "branch_on": (None, 1)}
    runs = {s: [] for s in sides}
    order = list(sides)
    for rep in range(repeats):
        for s in (order if rep % 2 == 0 else order[::-1]):
            lib, cov = sides[s]
            runs[s].append(run_json([sys.executable, os.path.abspath(__file__), "--child", gfa, str(n_reads), str(steps), str(warmup), str(cov)],
                                    env=lib_env(lib)))
            print(s, json.dumps(runs[s][-1]), file=sys.stderr, flush=True)
    rate = {s: [r["aligned_reads_per_s"] for r in runs[s]] for s in runs}
    mean = lambda v: sum(v) / len(v)
    on = runs["branch_on"]
    busy = {n: round(mean([r["busy_ms_per_step"][n] for r in on]), 3) for n in BUSY}
    return {"reads": n_reads, "steps": steps, "aligned_reads_per_s": rate,
            "slowdown_on_vs_parent": round(1.0 - mean(rate["branch_on"]) / mean(rate["parent"]), 4),
            "slowdown_off_vs_parent": round(1.0 - mean(rate["branch_off"]) / mean(rate["parent"]), 4),
            "busy_ms_per_step_counting_on": busy, "k_cov_runs_over_poa_text": round(busy["k_cov_runs"] / max(busy["poa_text"], 1e-9), 3),
            "counted": on[-1].get("counted")}


def cli(gfa, n_reads, repeats):
    import __graft_entry__ as ge

    p = ge.load_package()
    exe = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
    out = {"reads": n_reads, "modes": {}}
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        fa = os.path.join(d, "reads.fa")
        p.readsim.write_fasta(p.readsim.config3_reads(gfa, n_reads), fa)
        subprocess.check_call([exe, "index", "-i", gfa, "-k", "11", "-o", os.path.join(d, "ix")])
        modes = {"also_align": [], "coverage": ["--coverage"], "coverage_only": ["--coverage-only"]}
        for m in modes:
            out["modes"][m] = {"map_s": []}
        for rep in range(repeats):
            for m in (list(modes) if rep % 2 == 0 else list(modes)[::-1]):
                pre = os.path.join(d, "out_" + m)
                t0 = time.perf_counter()
                pr = subprocess.run([exe, "map", "-i", os.path.join(d, "ix"), "-f", fa, "-p", "abpoa", "-D", "-G", gfa, "-o", pre] + modes[m],
                                    capture_output=True, text=True)
                dt = time.perf_counter() - t0
                assert pr.returncode == 0, pr.stderr[-600:]
                o = out["modes"][m]
                o["map_s"].append(round(dt, 2))
                size = lambda sfx: os.path.getsize(pre + sfx) if os.path.exists(pre + sfx) else 0
                o["alignments_gaf_mb"] = round(size("-alignments.gaf") / 1e6, 1)
                o["chains_gaf_mb"] = round(size("-chains.gaf") / 1e6, 1)
                o["coverage_tsv_mb"] = round(sum(size("-coverage-%s.tsv" % t) for t in ("nodes", "bases", "edges")) / 1e6, 2)
                for sfx in ("-alignments.gaf", "-chains.gaf"):
                    if os.path.exists(pre + sfx):
                        os.remove(pre + sfx)
                print(m, dt, file=sys.stderr, flush=True)
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        gfa, n, steps, warmup, cov = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        return child_step(gfa, n, steps, warmup, cov)
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parts", default="bench_ab,step,cli")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cli-reads", type=int, default=100000)
    ap.add_argument("--cli-repeats", type=int, default=2)
    a = ap.parse_args()
    import __graft_entry__ as ge

    p = ge.load_package()
    parts = a.parts.split(",")
    if ("bench_ab" in parts or "step" in parts) and not a.parent_lib:
        ap.error("bench_ab and step compare against the parent commit: --parent-lib")
    cfg5 = os.path.join(tempfile.mkdtemp(prefix="vga_coverage_"), "config5.gfa")
    if "step" in parts or "cli" in parts:
        p.readsim.synth_pangenome(cfg5)
    res = {"command": "python tests/prof_coverage.py " + " ".join(x for x in sys.argv[1:] if not x.startswith("/")), "repeats": a.repeats}
    if "bench_ab" in parts:
        res["bench_ab"] = bench_ab(a.parent_lib, a.repeats)
    if "step" in parts:
        res["step"] = {"config3": step(a.parent_lib, DRB1, a.reads, a.steps, a.warmup, a.repeats),
                       "config5": step(a.parent_lib, cfg5, a.reads, a.steps, a.warmup, a.repeats)}
    if "cli" in parts:
        res["cli"] = {"config5": cli(cfg5, a.cli_reads, a.cli_repeats)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
