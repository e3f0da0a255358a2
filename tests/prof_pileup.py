"""diagnostic: what counting the pileup costs.  One JSON object on stdout (profiles/pileup.json).
Every measurement runs in a child process of its own, and the sides alternate, so that all sides of a comparison see the same
box in the same minutes.  `--parent-lib` names a libvga_hip.so built from the parent commit (the binding's VGA_LIB).

  step   config 3 and config 5 steps (10 000 x 10 kbp reads, seed 77: map + align, the step bench.py times) with the parent's
         library, with this one and the pileup off, and with this one counting, alternating; aligned reads/s and, from
         vga_last_kernel_times, the busy time per step of k_pu_events, k_pu_add and poa_text (k_poa_text) in the same runs.
         Off: the reads/s ranges of parent and branch_off must overlap.  On: the slowdown, and k_pu_events beside poa_text.

    python tests/prof_pileup.py --parent-lib PATH [--repeats 4] [--reads 10000] [--steps 3] [--configs config3,config5]
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
BUSY = ("k_pu_events", "k_pu_add", "poa_text", "poa_band_dp")


def child_step(gfa, n_reads, steps, warmup, pileup):
    """one process: reads/s of the timed steps and the kernels' busy time per step"""
    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(gfa, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(gfa, n_reads)])
    if pileup:
        ctx.pileup_begin()
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
    if pileup:
        t1 = time.perf_counter()
        counts, n_al, leading = ctx.pileup()
        out["read_ms"] = round((time.perf_counter() - t1) * 1e3, 2)
        out["counted"] = {"alignments": n_al, "leading_ins": leading, "graph_bases": int(counts.shape[0]),
                          "columns": dict(zip(p.binding.PILEUP_COLUMNS, (int(x) for x in counts.sum(0, dtype="uint64"))))}
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


def step(parent_lib, gfa, n_reads, steps, warmup, repeats):
    sides = {"parent": (parent_lib, 0), "branch_off": (None, 0), "branch_on": (None, 1)}
    runs = {s: [] for s in sides}
    order = list(sides)
    for rep in range(repeats):
        for s in (order if rep % 2 == 0 else order[::-1]):
            lib, on = sides[s]
            runs[s].append(run_json([sys.executable, os.path.abspath(__file__), "--child", gfa, str(n_reads), str(steps), str(warmup), str(on)],
                                    env=lib_env(lib)))
            print(s, json.dumps(runs[s][-1]), file=sys.stderr, flush=True)
    rate = {s: [r["aligned_reads_per_s"] for r in runs[s]] for s in runs}
    mean = lambda v: sum(v) / len(v)
    on = runs["branch_on"]
    busy = {n: round(mean([r["busy_ms_per_step"][n] for r in on]), 3) for n in BUSY}
    lo_b, hi_b, lo_p, hi_p = min(rate["branch_off"]), max(rate["branch_off"]), min(rate["parent"]), max(rate["parent"])
    return {"reads": n_reads, "steps": steps, "aligned_reads_per_s": rate,
            "off_ranges_overlap": bool(lo_b <= hi_p and lo_p <= hi_b),
            "slowdown_off_vs_parent": round(1.0 - mean(rate["branch_off"]) / mean(rate["parent"]), 4),
            "slowdown_on_vs_parent": round(1.0 - mean(rate["branch_on"]) / mean(rate["parent"]), 4),
            "busy_ms_per_step_counting_on": busy, "k_pu_events_over_poa_text": round(busy["k_pu_events"] / max(busy["poa_text"], 1e-9), 3),
            "read_ms": [r["read_ms"] for r in on], "counted": on[-1].get("counted")}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        gfa, n, steps, warmup, on = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        return child_step(gfa, n, steps, warmup, on)
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="config3,config5")
    a = ap.parse_args()
    import __graft_entry__ as ge

    p = ge.load_package()
    configs = a.configs.split(",")
    gfas = {"config3": DRB1}
    if "config5" in configs:
        gfas["config5"] = os.path.join(tempfile.mkdtemp(prefix="vga_pileup_"), "config5.gfa")
        p.readsim.synth_pangenome(gfas["config5"])
    res = {"command": "python tests/prof_pileup.py " + " ".join(x for x in sys.argv[1:] if not x.startswith("/")), "repeats": a.repeats, "step": {}}
    for c in configs:
        res["step"][c] = step(a.parent_lib, gfas[c], a.reads, a.steps, a.warmup, a.repeats)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
