"""diagnostic: what the store of the path abundance and its estimate cost.  One JSON object on stdout
(profiles/path_abundance.json).  Every measurement runs in a child process of its own with a time limit of its own, and the sides of
a comparison alternate, so that both see the same box in the same minutes; the first child that fails ends the script.
`--parent-lib` names a libvga_hip.so built from the parent commit by the same compiler (the binding's VGA_LIB).

  bench_ab   the switch off costs nothing: `python bench.py --gpus 1 --steps 3 --warmup 1` (config 3) with this tree's library and
             with the parent's, alternating, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  seam       vga_path_abundance_rows on `--rows` rows of random deficit bytes at 12, 256 and 4 096 paths, 32 iterations (one block,
             so every launch is a timed one): k_ab_estep and k_ab_mstep per iteration, k_ab_count, the wall time of the whole call,
             beside k_gl_pairs (vga_genotype_lik_pairs) on matrices of the same shape.
  step       one process: config 3 steps (10 000 x 10 kbp reads: map + align) with path support scored, without and with the store,
             alternating: reads/s of each step and k_ab_keep's time in it (a step with a fresh store pays its growth); then one
             store filled over `--steps` steps and the one estimate call at the end of such a run, three times.

    python tests/prof_path_abundance.py --parent-lib PATH [--parts bench_ab,seam,step] [--repeats 3] [--rows 10000] [--steps 4]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DRB1 = os.path.join(ROOT, "tests", "golden", "data", "DRB1-3123.gfa")
SEAM_PATHS = (12, 256, 4096)
SEAM_ITERS = 32
CHILD_LIMIT = {"bench": 600, "step": 600, "seam": 600}


def kernel_ms(ctx, prefixes):
    return {t["name"]: {"ms": round(t["ms"], 4), "launches": t["launches"]} for t in ctx.kernel_times() if t["name"].startswith(prefixes)}


def timed(ctx, call, prefixes, repeats=3):
    """the call once to warm up, then `repeats` times: wall time and the kernels of each -> (last result, runs)"""
    got = call()
    runs = []
    for _ in range(repeats):
        t1 = time.perf_counter()
        got = call()
        runs.append({"call_wall_ms": round((time.perf_counter() - t1) * 1e3, 2), "kernels": kernel_ms(ctx, prefixes)})
    return got, runs


def per_iteration(runs):
    """the timed launches of k_ab_estep and k_ab_mstep of every run, in microseconds per launch (a launch behind the last iteration
    returns at once and is among them: `iterations` beside it says how many did the work)"""
    out = {}
    for k in ("k_ab_estep", "k_ab_mstep"):
        out[k + "_us_per_iteration"] = [round(1e3 * r["kernels"][k]["ms"] / r["kernels"][k]["launches"], 2) for r in runs if k in r["kernels"]]
    return out


def child_seam(n_rows):
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    ctx = p.Context(0)
    rng = np.random.default_rng(1)
    out = {"rows": n_rows, "iterations": SEAM_ITERS, "shapes": {}}
    for n_paths in SEAM_PATHS:
        d = rng.integers(0, 3, size=(n_rows, n_paths)).astype(np.uint8)  # (small deficits under a small lambda: no launch finds the estimate converged)
        sc = np.ones(n_rows, dtype=np.uint8)
        res, runs = timed(ctx, lambda: ctx.path_abundance_rows(d, sc, 64, SEAM_ITERS, 0), ("k_ab",))
        b = d.astype(np.uint32)
        _, gl_runs = timed(ctx, lambda: ctx.genotype_likelihood_pairs(64 - np.minimum(b, 64), np.zeros_like(b), 512, 64), ("k_gl",))
        out["shapes"]["%d paths" % n_paths] = dict(per_iteration(runs), iterations_run=res["iterations"], vga_path_abundance_rows=runs, vga_genotype_lik_pairs=gl_runs)
    print(json.dumps(out), flush=True)


def child_step(n_reads, steps, warmup):
    import __graft_entry__ as ge
    import path_support_ref

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(DRB1, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(DRB1, n_reads)])
    _, paths = path_support_ref.parse_gfa(DRB1)
    ctx.path_support_begin(*path_support_ref.packed_steps(paths))
    for _ in range(warmup):
        b.map_align_raw()

    def step():
        t1 = time.perf_counter()
        b.map_align_raw()
        ctx.synchronize()
        dt = time.perf_counter() - t1
        keep = [t for t in ctx.kernel_times() if t["name"] == "k_ab_keep"]
        return {"reads_per_s": round(n_reads / dt, 1), "k_ab_keep_busy_ms": round(keep[0]["busy_ms"], 4) if keep else None}

    sides = {"path_support_only": [], "with_the_store": []}
    for _ in range(steps):
        sides["path_support_only"].append(step())
        ctx.path_abundance_begin()
        sides["with_the_store"].append(step())  # (a fresh store each time: every one of these steps pays the growth)
        ctx.path_abundance_end()
    ctx.path_abundance_begin()
    grown = [step() for _ in range(steps)]      # (the store doubles as it fills: the later steps grow less often)
    d, sc = ctx.path_abundance_store()
    res, runs = timed(ctx, lambda: ctx.path_abundance(), ("k_ab",))
    out = {"rows_kept": int(len(sc)), "rows_scored": int(sc.sum()), "paths": int(d.shape[1]), "store_bytes": int(d.size + sc.size),
           "steps_alternating": sides, "steps_filling_one_store": grown, "iterations": res["iterations"], "converged": res["converged"],
           "ppm": [int(v) for v in p.binding.path_abundance_ppm(res["theta"])], "vga_path_abundance": runs}
    out.update(per_iteration(runs))
    print(json.dumps(out), flush=True)


def run_child(args, env=None, limit=600):
    import subprocess

    pr = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    if pr.returncode != 0:
        sys.stderr.write(pr.stdout[-2000:] + pr.stderr[-4000:])
        raise SystemExit("child failed (%d): %s" % (pr.returncode, " ".join(args)))
    print("done:", " ".join(args)[-100:], file=sys.stderr, flush=True)
    return json.loads([l for l in pr.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parts", default="bench_ab,seam,step")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child:
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        if a.child[0] == "seam":
            return child_seam(int(a.child[1]))
        return child_step(int(a.child[0]), int(a.child[1]), int(a.child[2]))
    me = os.path.abspath(__file__)
    out = {"what": "what the store and the estimate of the path abundance cost on one MI355X (DESIGN.md section 30); no figure here is asserted by a test"}
    parts = a.parts.split(",")
    env = dict(os.environ)
    env.pop("VGA_LIB", None)
    if "bench_ab" in parts:
        assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: a libvga_hip.so built from the parent commit"
        runs = {"branch": [], "parent": []}
        order = []
        for rep in range(a.repeats):
            for side in (("branch", "parent") if rep % 2 == 0 else ("parent", "branch")):  # (neither side always runs first)
                e = dict(env)
                if side == "parent":
                    e["VGA_LIB"] = os.path.abspath(a.parent_lib)
                order.append(side)
                runs[side].append(run_child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=e, limit=CHILD_LIMIT["bench"])["value"])
        rng = {s: [min(v), max(v)] for s, v in runs.items()}
        out["bench_ab"] = {"bench": "python bench.py --gpus 1 --steps 3 --warmup 1", "metric": "aligned reads/s, config 3", "order": order,
                           "runs": runs, "branch_range": rng["branch"], "parent_range": rng["parent"],
                           "ranges_overlap": rng["branch"][0] <= rng["parent"][1] and rng["parent"][0] <= rng["branch"][1]}
    if "seam" in parts:
        out["seam"] = run_child([me, "--child", "seam", str(a.rows)], env=env, limit=CHILD_LIMIT["seam"])
    if "step" in parts:
        out["step"] = dict(run_child([me, "--child", str(a.reads), str(a.steps), str(a.warmup)], env=env, limit=CHILD_LIMIT["step"]),
                           workload="config 3: %d reads of 10 kbp on DRB1-3123, path support scored" % a.reads)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
