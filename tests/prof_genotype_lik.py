"""diagnostic: what the genotype likelihood costs.  One JSON object on stdout (profiles/genotype_likelihood.json).
Every measurement runs in a child process of its own with a time limit of its own, and the processes of a pair alternate, so that
both sides of a comparison see the same box in the same minutes; the first child that fails ends the script.  `--parent-lib` names a
libvga_hip.so built from the parent commit by the same compiler (the binding's VGA_LIB).

  bench_ab   off costs nothing: `python bench.py --gpus 1 --steps 3 --warmup 1` (config 3) with this tree's library and with the
             parent's, alternating, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  many       both kernels alone through the seam vga_genotype_lik_pairs: `--reads` random rows against 16, 256, 1024 and 4096 paths,
             and k_gt_pairs through its own seam on the same matrices in the same process; kernel times from vga_last_kernel_times,
             pair-reads per second, and the VALU instructions of both inner loops counted in the cross-compiled ISA.
  step       the on-cost at a dozen paths: config 3 steps (10 000 x 10 kbp reads, seed 77: map + align, the step bench.py times)
             with path support on and with path support plus the likelihood on, same library, alternating.

    python tests/prof_genotype_lik.py --parent-lib PATH [--parts bench_ab,many,step] [--repeats 4] [--reads 10000] [--steps 3]
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
BUSY = ("k_ps_score", "k_gl_deficit", "k_gl_pairs", "poa_band_dp")
MIXED_VALU_PER_S = 0.58e12  # profiles/r02_valu_issue_microbench.txt: wave-instructions per second, mixed VALU, whole device


def inner_loop(source, kernel, lds_read, pair_reads_per_lane):
    """the innermost loop of `kernel` that reads LDS with `lds_read`, from a cross-compile: its instructions by kind"""
    csrc = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                               "--cuda-device-only", os.path.join(csrc, source), "-o", out], stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    begin = next(i for i, l in enumerate(lines) if re.match(r"_Z\w*\d+" + kernel + r"E\w*:", l))
    end = next(i for i in range(begin, len(lines)) if ".end_amdhsa_kernel" in lines[i])
    best = None
    for i in range(begin, end):
        m = re.match(r"(\.LBB\d+_\d+):", lines[i])
        if not m or "Inner Loop Header: Depth=2" not in lines[i + 1]:
            continue
        for j in range(i + 1, end):
            if re.search(r"s_cbranch_\w+\s+" + re.escape(m.group(1)) + r"\b", lines[j]):
                body = [x.strip() for x in lines[i + 1:j + 1]]
                if any(x.startswith(lds_read) for x in body):
                    best = body
                break
    assert best, "inner loop of %s not found" % kernel
    body = [x for x in best if x and not x.startswith((";", "."))]
    valu = sum(1 for x in body if x.startswith("v_"))
    return {"instructions": len(body), "valu": valu, "lds_reads": sum(1 for x in body if x.startswith("ds_read")),
            "waits": sum(1 for x in body if x.startswith("s_waitcnt")), "pair_reads_per_lane": pair_reads_per_lane,
            "valu_wave_instructions_per_64_pair_reads": round(valu / float(pair_reads_per_lane), 3),
            "lds_wave_instructions_per_64_pair_reads": round(sum(1 for x in body if x.startswith("ds_read")) / float(pair_reads_per_lane), 3)}


def child_many(n_reads):
    """one process: both seams at more and more paths, on the same matrices"""
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    b_ = p.binding
    ctx = p.Context(0)
    rng = np.random.default_rng(7)
    loops = {"k_gl_pairs": inner_loop("vga_genotype_lik.hip", "k_gl_pairs", "ds_read_u16", 64),
             "k_gt_pairs": inner_loop("vga_genotype.hip", "k_gt_pairs", "ds_read", 16)}
    rows = []
    for n_paths in (16, 256, 1024, 4096):
        b = rng.integers(0, 1 << 14, (n_reads, n_paths), dtype=np.uint32)
        e = rng.integers(0, 1 << 9, (n_reads, n_paths), dtype=np.uint32)
        # (random rows: nearly every deficit is at the cap; a second pair of matrices keeps them within 2 cap of the row's best)
        near = (b.max(axis=1, keepdims=True) - rng.integers(0, 2 * b_.GENOTYPE_LIK_CAP, b.shape)).astype(np.uint32)
        row = {"paths": n_paths, "pairs": n_paths * (n_paths + 1) // 2}
        for what, bb, ee in (("random", b, e), ("near", near, np.zeros_like(e))):
            ctx.genotype_likelihood_pairs(bb[:64], ee[:64])  # (warm-up: the code object, the allocator)
            t0 = time.perf_counter()
            t = ctx.genotype_likelihood_pairs(bb, ee)
            call_ms = (time.perf_counter() - t0) * 1e3
            ms = {k["name"]: k["ms"] for k in ctx.kernel_times()}
            tiles = (n_paths + b_.GENOTYPE_LIK_TILE - 1) // b_.GENOTYPE_LIK_TILE
            slots = tiles * (tiles + 1) // 2 * b_.GENOTYPE_LIK_TILE ** 2  # pair slots the launched tiles compute, useful or not
            s = ms["k_gl_pairs"] * 1e-3
            row[what] = {"k_gl_deficit_ms": round(ms["k_gl_deficit"], 4), "k_gl_pairs_ms": round(ms["k_gl_pairs"], 4), "call_ms": round(call_ms, 2),
                         "deficit_bytes_per_s": round(n_reads * n_paths * 17 / (ms["k_gl_deficit"] * 1e-3), 0),  # two passes over 8 bytes, one byte out
                         "pair_reads_per_s": round(row["pairs"] * n_reads / s, 0), "computed_pair_reads_per_s": round(slots * n_reads / s, 0),
                         "valu_wave_instructions_per_s": round(slots * n_reads / 64.0 * loops["k_gl_pairs"]["valu_wave_instructions_per_64_pair_reads"] / s, 0),
                         "fraction_of_mixed_valu_issue": round(slots * n_reads / 64.0 * loops["k_gl_pairs"]["valu_wave_instructions_per_64_pair_reads"] / s / MIXED_VALU_PER_S, 4),
                         "share_of_deficits_at_cap": round(float((t["deficit"] == b_.GENOTYPE_LIK_CAP).mean()), 4), "cost_sum": int(t["cost"].sum(dtype="uint64"))}
        ctx.genotype_pairs(b[:64], e[:64])
        ctx.genotype_pairs(b, e)
        gt = sum(k["ms"] for k in ctx.kernel_times() if k["name"] == "k_gt_pairs")
        row["k_gt_pairs_ms"] = round(gt, 4)
        row["k_gl_pairs_over_k_gt_pairs"] = round(row["random"]["k_gl_pairs_ms"] / gt, 4) if gt else None
        rows.append(row)
    print(json.dumps({"reads": n_reads, "lambda": b_.GENOTYPE_LIK_LAMBDA, "cap": b_.GENOTYPE_LIK_CAP, "inner_loops": loops, "rows": rows}), flush=True)


def child_step(gfa, n_reads, steps, warmup, on):
    """one process: reads/s of the timed steps and the kernels' busy time per step, path support on"""
    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(gfa, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(gfa, n_reads)])
    g = p.hostlib.gfa_paths(gfa)
    ctx.path_support_begin(g["step_off"], g["steps"])
    if on:
        ctx.genotype_likelihood_begin()
    for _ in range(warmup):
        b.map_align_raw()
    ctx.synchronize()
    ctx.path_support_reset()
    if on:
        ctx.genotype_likelihood_reset()
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
    if on:
        t = ctx.genotype_likelihood()
        best = p.binding.genotype_likelihood_rank(t["cost"], t["n_paths"], 2)
        out["table"] = {"pairs": len(t["cost"]), "n_scored": t["n_scored"], "best": [g["names"][i] for i in best[0][:2]], "cost": best[0][2], "next": best[1][3]}
    print(json.dumps(out), flush=True)


def run_json(cmd, env=None, timeout=600):
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


BENCH = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]


def bench_ab(parent_lib, repeats):
    vals = {"branch": [], "parent": []}
    kernels = {"branch": [], "parent": []}
    for rep in range(repeats):
        for side in (("branch", "parent") if rep % 2 == 0 else ("parent", "branch")):
            line = run_json([sys.executable, os.path.join(ROOT, BENCH[0])] + BENCH[1:], env=lib_env(parent_lib if side == "parent" else None))
            vals[side].append(line["value"])
            kernels[side].append({k: v for k, v in line.items() if "kernel" in k})
            print(side, line["value"], file=sys.stderr, flush=True)
    lo_b, hi_b, lo_p, hi_p = min(vals["branch"]), max(vals["branch"]), min(vals["parent"]), max(vals["parent"])
    out = {"command": "python " + " ".join(BENCH), "metric": "aligned reads/s, config 3", "runs": vals, "branch_range": [lo_b, hi_b], "parent_range": [lo_p, hi_p],
           "ranges_overlap": bool(lo_b <= hi_p and lo_p <= hi_b), "branch_best_below_parent_worst": bool(hi_b < lo_p)}
    if not out["ranges_overlap"]:
        out["per_kernel"] = kernels
    return out


def step(gfa, n_reads, steps, warmup, repeats):
    runs = {"path_support": [], "likelihood": []}
    for rep in range(repeats):
        for s in (("path_support", "likelihood") if rep % 2 == 0 else ("likelihood", "path_support")):
            runs[s].append(run_json([sys.executable, os.path.abspath(__file__), "--child", gfa, str(n_reads), str(steps), str(warmup),
                                     "1" if s == "likelihood" else "0"], env=lib_env(None)))
            print(s, json.dumps(runs[s][-1]), file=sys.stderr, flush=True)
    mean = lambda v: sum(v) / len(v)
    rate = {s: [r["aligned_reads_per_s"] for r in runs[s]] for s in runs}
    on = runs["likelihood"]
    busy = {n: round(mean([r["busy_ms_per_step"][n] for r in on]), 4) for n in BUSY}
    return {"reads": n_reads, "steps": steps, "paths": on[-1]["paths"], "aligned_reads_per_s": rate,
            "ms_per_step": {s: [r["ms_per_step"] for r in runs[s]] for s in runs},
            "slowdown_likelihood_vs_path_support": round(1.0 - mean(rate["likelihood"]) / mean(rate["path_support"]), 4),
            "busy_ms_per_step_likelihood": busy, "table": on[-1]["table"]}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        gfa, n, steps, warmup, on = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        return child_step(gfa, n, steps, warmup, on)
    if len(sys.argv) > 1 and sys.argv[1] == "--child-many":
        return child_many(int(sys.argv[2]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parts", default="bench_ab,many,step")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    parts = a.parts.split(",")
    if "bench_ab" in parts and not a.parent_lib:
        ap.error("bench_ab compares against the parent commit: --parent-lib")
    res = {"command": "python tests/prof_genotype_lik.py " + " ".join(x for x in sys.argv[1:] if not x.startswith("/")), "repeats": a.repeats}
    if "many" in parts:
        res["many"] = run_json([sys.executable, os.path.abspath(__file__), "--child-many", str(a.reads)], env=lib_env(None))
    if "step" in parts:
        res["step"] = {"config3": step(DRB1, a.reads, a.steps, a.warmup, a.repeats)}
    if "bench_ab" in parts:
        res["bench_ab"] = bench_ab(os.path.abspath(a.parent_lib), a.repeats)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
