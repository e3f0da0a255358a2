"""diagnostic: what counting and calling the inserted letters costs.  One JSON object on stdout
(profiles/insertion_calls.json).  Every measurement runs in a child process of its own with a time limit of its own, and the sides
of a comparison alternate, so that both see the same box in the same minutes; the first child that fails ends the script.
`--parent-lib` names a libvga_hip.so built from the parent commit by the same compiler (the binding's VGA_LIB).

  bench_ab   the switch off costs nothing: `python bench.py --gpus 1 --steps 3 --warmup 1` (config 3) with this tree's library and
             with the parent's, alternating, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  step       config 3 steps (10 000 x 10 kbp reads: map + align, the step bench.py times) counting the pileup alone -- what
             --call-variants turns on -- and counting the insertion table too -- --call-insertions --, alternating: aligned reads/s
             and, from vga_last_kernel_times, the busy time per step of k_pu_events, k_pu_add, k_ia_events, k_ia_add and poa_text.
             The side that counts both then calls the variants, and the insertions at the sites reported het or hom: k_ia_call
             through vga_insertion_call and, on the same rows, through the seam vga_insertion_call_table.

    python tests/prof_insertion.py --parent-lib PATH [--parts bench_ab,step] [--repeats 3] [--reads 10000] [--steps 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRB1 = os.path.join(ROOT, "tests", "golden", "data", "DRB1-3123.gfa")
BUSY = ("k_pu_events", "k_pu_add", "k_ia_events", "k_ia_add", "poa_text", "poa_band_dp")


def child_step(n_reads, steps, warmup, insertions):
    """one process: reads/s of the timed steps and the kernels' busy time per step; with `insertions` the calls behind them"""
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(DRB1, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(DRB1, n_reads)])
    ctx.pileup_begin()
    if insertions:
        ctx.insertion_begin()
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
    if insertions:
        calls = ctx.variant_call()
        pos = calls["pos"][calls["ins"] > 0]
        kernel = lambda: round({t["name"]: t["ms"] for t in ctx.kernel_times()}["k_ia_call"], 4) if len(pos) else None
        ctx.insertion_call(pos)  # (warm-up)
        own, seam = [], []
        for _ in range(5):
            t1 = time.perf_counter()
            got = ctx.insertion_call(pos)
            own.append({"call_wall_ms": round((time.perf_counter() - t1) * 1e3, 3), "k_ia_call_ms": kernel()})
            t1 = time.perf_counter()
            ctx.insertion_call_table(got["rows"])
            seam.append({"call_wall_ms": round((time.perf_counter() - t1) * 1e3, 3), "k_ia_call_ms": kernel()})
        t1 = time.perf_counter()
        counts, n_al, n_ev, n_leading = ctx.insertions()
        out["read_ms"] = round((time.perf_counter() - t1) * 1e3, 2)
        out["counted"] = {"alignments": n_al, "insertions": n_ev, "leading": n_leading, "graph_bases": int(counts.shape[0]),
                          "bases_with_an_insertion": int(np.count_nonzero(counts[:, :9].sum(1))),
                          "longer_than_8": int(counts[:, 8].sum(dtype="uint64"))}
        out["call"] = {"variant_calls": int(calls["n_calls"]), "sites": int(len(pos)), "sites_longer_than_8": int((got["length"] > 8).sum()) if len(pos) else 0,
                       "vga_insertion_call": own, "vga_insertion_call_table": seam}
    print(json.dumps(out), flush=True)


def run_child(args, env=None, limit=600):
    pr = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    if pr.returncode != 0:
        sys.stderr.write(pr.stdout[-2000:] + pr.stderr[-4000:])
        raise SystemExit("child failed (%d): %s" % (pr.returncode, " ".join(args)))
    print("done:", " ".join(args)[-100:], file=sys.stderr, flush=True)
    return json.loads([l for l in pr.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parts", default="bench_ab,step")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child:
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        return child_step(int(a.child[0]), int(a.child[1]), int(a.child[2]), int(a.child[3]))
    me = os.path.abspath(__file__)
    out = {"what": "what counting and calling the inserted letters costs on one MI355X (DESIGN.md section 22); no figure here is asserted by a test"}
    parts = a.parts.split(",")
    mean = lambda v: sum(v) / len(v)
    if "step" in parts:
        env = dict(os.environ)
        env.pop("VGA_LIB", None)
        runs = {"pileup": [], "pileup_and_insertions": []}
        for rep in range(a.repeats):
            for side in (list(runs) if rep % 2 == 0 else list(runs)[::-1]):
                runs[side].append(run_child([me, "--child", str(a.reads), str(a.steps), str(a.warmup), str(int(side != "pileup"))], env=env))
        rate = {s: [r["aligned_reads_per_s"] for r in runs[s]] for s in runs}
        on = runs["pileup_and_insertions"]
        busy = {n: round(mean([r["busy_ms_per_step"][n] for r in on]), 3) for n in BUSY}
        out["step"] = {"workload": "config 3: %d reads of 10 kbp on DRB1-3123, %d timed steps after %d" % (a.reads, a.steps, a.warmup),
                       "aligned_reads_per_s": rate, "ms_per_step": {s: [r["ms_per_step"] for r in runs[s]] for s in runs},
                       "slowdown_with_insertions": round(1.0 - mean(rate["pileup_and_insertions"]) / mean(rate["pileup"]), 4),
                       "busy_ms_per_step_counting_both": busy,
                       "k_ia_events_over_k_pu_events": round(busy["k_ia_events"] / max(busy["k_pu_events"], 1e-9), 3),
                       "read_ms": [r["read_ms"] for r in on], "counted": on[-1]["counted"], "call": on[-1]["call"]}
    if "bench_ab" in parts:
        assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: a libvga_hip.so built from the parent commit"
        runs = {"branch": [], "parent": []}
        for _ in range(a.repeats):
            for side in ("branch", "parent"):
                env = dict(os.environ)
                env.pop("VGA_LIB", None)
                if side == "parent":
                    env["VGA_LIB"] = os.path.abspath(a.parent_lib)
                runs[side].append(run_child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env)["value"])
        rng = {s: [min(v), max(v)] for s, v in runs.items()}
        out["bench_ab"] = {"bench": "python bench.py --gpus 1 --steps 3 --warmup 1", "metric": "aligned reads/s, config 3",
                           "order": "branch and parent alternating, processes of their own, one box; the parent's library built from the parent commit with the same compiler (VGA_LIB)",
                           "runs": runs, "branch_range": rng["branch"], "parent_range": rng["parent"],
                           "ranges_overlap": rng["branch"][0] <= rng["parent"][1] and rng["parent"][0] <= rng["branch"][1]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
