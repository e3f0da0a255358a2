"""diagnostic: what genotyping costs.  One JSON object on stdout (profiles/genotype.json).
Every measurement runs in a child process of its own, and the processes of a pair alternate, so that both sides of a comparison
see the same box in the same minutes.  `--parent-lib` names a libvga_hip.so built from the parent commit (the binding's VGA_LIB).

  bench_ab   off costs nothing: `python bench.py` (config 3) with this tree's library and with the parent's, alternating,
             `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  step       the on-cost: config 3 (12 paths) and config 5 (16 paths) steps (10 000 x 10 kbp reads, seed 77: map + align, the step
             bench.py times) with path support on and with path support plus genotyping on, same library, alternating; aligned
             reads/s and, from vga_last_kernel_times, the busy time per step of k_gt_pairs beside k_ps_score.
  many       the kernel alone through the seam vga_genotype_pairs: `--reads` random rows against 16, 64, 256, 1024 and 4096 paths;
             kernel time, pair-reads per second, and -- with the VALU instructions of the inner loop counted in the kernel's ISA --
             VALU wave-instructions per second against the 0.58 T/s of profiles/r02_valu_issue_microbench.txt.

    python tests/prof_genotype.py --parent-lib PATH [--parts bench_ab,step,many] [--repeats 4] [--reads 10000] [--steps 3]
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
BUSY = ("k_cov_runs", "k_ps_score", "k_gt_pairs", "poa_band_dp")
MIXED_VALU_PER_S = 0.58e12  # profiles/r02_valu_issue_microbench.txt: wave-instructions per second, mixed VALU, whole device


def child_step(gfa, n_reads, steps, warmup, genotype):
    """one process: reads/s of the timed steps and the kernels' busy time per step, path support on"""
    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(gfa, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(gfa, n_reads)])
    g = p.hostlib.gfa_paths(gfa)
    ctx.path_support_begin(g["step_off"], g["steps"])
    if genotype:
        ctx.genotype_begin()
    for _ in range(warmup):
        b.map_align_raw()
    ctx.synchronize()
    ctx.path_support_reset()
    if genotype:
        ctx.genotype_reset()
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
    out = {"paths": len(g["names"]), "aligned_reads_per_s": round(aligned / dt, 1), "ms_per_step": round(dt / steps * 1e3, 1),
           "busy_ms_per_step": {n: round(v / steps, 4) for n, v in busy.items()}}
    if genotype:
        t = ctx.genotype()
        best = p.binding.genotype_rank(t, 1)
        out["table"] = {"pairs": len(t["sum_bases"]), "sum_bases": int(t["sum_bases"].sum()), "sum_edges": int(t["sum_edges"].sum()),
                        "prefer_a": int(t["prefer_a"].sum()), "prefer_b": int(t["prefer_b"].sum()),
                        "best": [g["names"][i] for i in best[0]] if best else None}
    print(json.dumps(out), flush=True)


def inner_loop_valu():
    """VALU instructions of k_gt_pairs' inner loop (one read, the 16 pairs of a lane) from a cross-compile, per 64 pair-reads"""
    csrc = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "gt.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                               "--cuda-device-only", os.path.join(csrc, "vga_genotype.hip"), "-o", out], stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    # the innermost loop: the deepest "Inner Loop Header" block that reads LDS, up to its backward branch
    best = None
    for i, l in enumerate(lines):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if not m or i + 1 >= len(lines) or "Inner Loop Header: Depth=2" not in lines[i + 1]:
            continue
        for j in range(i + 1, len(lines)):
            if re.search(r"s_cbranch_\w+\s+" + re.escape(m.group(1)) + r"\b", lines[j]):
                body = [x.strip() for x in lines[i + 1:j + 1]]
                if any(x.startswith("ds_read") for x in body):
                    best = body
                break
    assert best, "inner loop not found"
    valu = sum(1 for x in best if x.startswith("v_"))
    return {"instructions": len([x for x in best if x and not x.startswith((";", "."))]), "valu": valu, "lds_reads": sum(1 for x in best if x.startswith("ds_read")),
            "pair_reads_per_lane": 16, "valu_wave_instructions_per_64_pair_reads": round(valu / 16.0, 3)}


def child_many(n_reads):
    """one process: the seam at more and more paths"""
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    ctx = p.Context(0)
    rng = np.random.default_rng(7)
    loop = inner_loop_valu()
    rows = []
    for n_paths in (16, 64, 256, 1024, 4096):
        b = rng.integers(0, 1 << 14, (n_reads, n_paths), dtype=np.uint32)
        e = rng.integers(0, 1 << 9, (n_reads, n_paths), dtype=np.uint32)
        ctx.genotype_pairs(b[:64], e[:64])  # (warm-up: the code object, the allocator)
        t0 = time.perf_counter()
        t = ctx.genotype_pairs(b, e)
        call_ms = (time.perf_counter() - t0) * 1e3
        ms = sum(k["ms"] for k in ctx.kernel_times() if k["name"] == "k_gt_pairs")
        pairs = n_paths * (n_paths + 1) // 2
        tiles = (n_paths + p.binding.GENOTYPE_TILE - 1) // p.binding.GENOTYPE_TILE
        slots = tiles * (tiles + 1) // 2 * p.binding.GENOTYPE_TILE ** 2  # pair slots the launched tiles compute, useful or not
        rows.append({"paths": n_paths, "pairs": pairs, "k_gt_pairs_ms": round(ms, 4), "call_ms": round(call_ms, 2),
                     "pair_reads_per_s": round(pairs * n_reads / (ms * 1e-3), 0) if ms else None,
                     "computed_pair_reads_per_s": round(slots * n_reads / (ms * 1e-3), 0) if ms else None,
                     "valu_wave_instructions_per_s": round(slots * n_reads / 64.0 * loop["valu_wave_instructions_per_64_pair_reads"] / (ms * 1e-3), 0) if ms else None,
                     "fraction_of_mixed_valu_issue": round(slots * n_reads / 64.0 * loop["valu_wave_instructions_per_64_pair_reads"] / (ms * 1e-3) / MIXED_VALU_PER_S, 4) if ms else None,
                     "sum_bases": int(t["sum_bases"].sum(dtype="uint64"))})
    print(json.dumps({"reads": n_reads, "inner_loop": loop, "rows": rows}), flush=True)


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


def step(gfa, n_reads, steps, warmup, repeats):
    runs = {"path_support": [], "genotype": []}
    for rep in range(repeats):
        for s in (("path_support", "genotype") if rep % 2 == 0 else ("genotype", "path_support")):
            runs[s].append(run_json([sys.executable, os.path.abspath(__file__), "--child", gfa, str(n_reads), str(steps), str(warmup),
                                     "1" if s == "genotype" else "0"], env=lib_env(None)))
            print(s, json.dumps(runs[s][-1]), file=sys.stderr, flush=True)
    mean = lambda v: sum(v) / len(v)
    rate = {s: [r["aligned_reads_per_s"] for r in runs[s]] for s in runs}
    on = runs["genotype"]
    busy = {n: round(mean([r["busy_ms_per_step"][n] for r in on]), 4) for n in BUSY}
    return {"reads": n_reads, "steps": steps, "paths": on[-1]["paths"], "aligned_reads_per_s": rate,
            "ms_per_step": {s: [r["ms_per_step"] for r in runs[s]] for s in runs},
            "slowdown_genotype_vs_path_support": round(1.0 - mean(rate["genotype"]) / mean(rate["path_support"]), 4),
            "busy_ms_per_step_genotype": busy, "k_gt_pairs_over_k_ps_score": round(busy["k_gt_pairs"] / busy["k_ps_score"], 4) if busy["k_ps_score"] else None,
            "table": on[-1]["table"]}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        gfa, n, steps, warmup, on = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        return child_step(gfa, n, steps, warmup, on)
    if len(sys.argv) > 1 and sys.argv[1] == "--child-many":
        return child_many(int(sys.argv[2]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parts", default="bench_ab,step,many")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import __graft_entry__ as ge

    p = ge.load_package()
    parts = a.parts.split(",")
    if "bench_ab" in parts and not a.parent_lib:
        ap.error("bench_ab compares against the parent commit: --parent-lib")
    res = {"command": "python tests/prof_genotype.py " + " ".join(x for x in sys.argv[1:] if not x.startswith("/")), "repeats": a.repeats}
    if "many" in parts:
        res["many"] = run_json([sys.executable, os.path.abspath(__file__), "--child-many", str(a.reads)], env=lib_env(None))
    if "step" in parts:
        cfg5 = os.path.join(tempfile.mkdtemp(prefix="vga_genotype_"), "config5.gfa")
        p.readsim.synth_pangenome(cfg5)
        res["step"] = {"config3": step(DRB1, a.reads, a.steps, a.warmup, a.repeats), "config5": step(cfg5, a.reads, a.steps, a.warmup, a.repeats)}
    if "bench_ab" in parts:
        res["bench_ab"] = bench_ab(os.path.abspath(a.parent_lib), a.repeats)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
