"""diagnostic: the list makers before and after a change to what they share in vga_oplist.hpp -- their walk (DESIGN.md sections 13
and 16, profiles/oplist_shared_ab.json) and their host frame (section 27, profiles/oplist_stage_ab.json).  One JSON object on
stdout.  Every measurement runs in a child process of its own, under a time limit of
its own, and the sides alternate, so that both sides of the comparison see the same box in the same minutes; the script stops
at the first child that fails.  `--parent-lib` names a libvga_hip.so built from the parent commit (the binding's VGA_LIB).

  step   config 3 and config 5 steps (10 000 x 10 kbp reads, seed 77: map + align, the step bench.py times) with coverage, the
         pileup, the insertion table and path support all counting, with the parent's library (parent_on) and with this one
         (branch_on), alternating.  Per run: aligned reads/s, the wall time of a step, from vga_last_kernel_times the busy time
         per step of the makers' list and add kernels and of poa_text (k_poa_text), and a SHA-256 over the bytes of every table
         read back.  The digests of the two sides must be equal; for each of the walk kernels the branch's median must not exceed
         the parent's slowest run; `in_parent_range` says for every kernel and for the step whether the branch's median lies
         inside the parent's own fastest-to-slowest range.

    python tests/prof_oplist_ab.py --parent-lib PATH [--repeats 3] [--reads 10000] [--steps 3] [--configs config3,config5]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRB1 = os.path.join(ROOT, "tests", "golden", "data", "DRB1-3123.gfa")
BUSY = ("k_cov_runs", "k_pu_events", "k_ia_events", "k_cov_add", "k_pu_add", "k_ia_add", "poa_text")
WALK = ("k_cov_runs", "k_pu_events", "k_ia_events")
ACC = ("sum_bases", "sum_edges", "top", "top_alone")


def child_step(gfa, n_reads, steps, warmup):
    """one process: reads/s of the timed steps, the kernels' busy time per step and the digest of the tables"""
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(gfa, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(gfa, n_reads)])
    g = p.hostlib.gfa_paths(gfa)
    ctx.coverage_begin()
    ctx.pileup_begin()
    ctx.insertion_begin()
    ctx.path_support_begin(g["step_off"], g["steps"])
    for _ in range(warmup):
        b.map_align_raw()
    ctx.synchronize()
    ctx.coverage_reset()
    ctx.pileup_reset()
    ctx.insertion_reset()
    ctx.path_support_reset()
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
    base, node, edge, n_cov = ctx.coverage()
    counts, n_pu, leading = ctx.pileup()
    ins, n_ia, n_events, n_leading = ctx.insertions()
    acc = ctx.path_support()
    h = hashlib.sha256()
    for a in (base, node, edge, counts, np.array([n_pu, leading], dtype=np.uint64), ins, np.array([n_ia, n_events, n_leading], dtype=np.uint64)) + tuple(acc[k] for k in ACC):
        h.update(np.ascontiguousarray(a).tobytes())
    print(json.dumps({"aligned_reads_per_s": round(aligned / dt, 1), "ms_per_step": round(dt / steps * 1e3, 1),
                      "busy_ms_per_step": {n: round(v / steps, 3) for n, v in busy.items()}, "tables_sha256": h.hexdigest(),
                      "counted": {"coverage": n_cov, "pileup": n_pu, "leading_ins": leading, "insertions": n_ia, "insertion_events": n_events, "path_support": acc["n_alignments"]}}), flush=True)


def run_json(cmd, env, timeout):
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


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else (s[len(s) // 2 - 1] + s[len(s) // 2]) / 2


def step(parent_lib, gfa, n_reads, steps, warmup, repeats, timeout):
    sides = {"parent_on": parent_lib, "branch_on": None}
    runs = {s: [] for s in sides}
    order = list(sides)
    for rep in range(repeats):
        for s in (order if rep % 2 == 0 else order[::-1]):
            # (a child that fails or runs out of time raises: nothing more is started)
            runs[s].append(run_json([sys.executable, os.path.abspath(__file__), "--child", gfa, str(n_reads), str(steps), str(warmup)],
                                    lib_env(sides[s]), timeout))
            print(s, json.dumps(runs[s][-1]), file=sys.stderr, flush=True)
    digests = {s: sorted({r["tables_sha256"] for r in runs[s]}) for s in runs}
    busy = {s: {n: [r["busy_ms_per_step"][n] for r in runs[s]] for n in BUSY} for s in runs}
    walk = {n: {"parent_slowest": max(busy["parent_on"][n]), "branch_median": median(busy["branch_on"][n])} for n in WALK}
    for n in WALK:
        walk[n]["branch_median_not_above_parent_slowest"] = bool(walk[n]["branch_median"] <= walk[n]["parent_slowest"])
    wall = {s: [r["ms_per_step"] for r in runs[s]] for s in runs}
    in_range = {n: bool(min(v["parent_on"]) <= median(v["branch_on"]) <= max(v["parent_on"]))
                for n, v in [(n, {s: busy[s][n] for s in runs}) for n in BUSY] + [("ms_per_step", wall)]}
    return {"reads": n_reads, "steps": steps, "aligned_reads_per_s": {s: [r["aligned_reads_per_s"] for r in runs[s]] for s in runs}, "ms_per_step": wall,
            "busy_ms_per_step": busy, "walk_kernels": walk, "in_parent_range": in_range, "tables_sha256": digests,
            "tables_equal": bool(digests["parent_on"] == digests["branch_on"] and len(digests["branch_on"]) == 1),
            "counted": runs["branch_on"][-1]["counted"]}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        return child_step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="config3,config5")
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds a measurement may take")
    a = ap.parse_args()
    import __graft_entry__ as ge

    p = ge.load_package()
    configs = a.configs.split(",")
    gfas = {"config3": DRB1}
    if "config5" in configs:
        gfas["config5"] = os.path.join(tempfile.mkdtemp(prefix="vga_oplist_"), "config5.gfa")
        p.readsim.synth_pangenome(gfas["config5"])
    res = {"command": "python tests/prof_oplist_ab.py " + " ".join(x for x in sys.argv[1:] if not x.startswith("/")), "repeats": a.repeats, "step": {}}
    for c in configs:
        res["step"][c] = step(a.parent_lib, gfas[c], a.reads, a.steps, a.warmup, a.repeats, a.child_timeout)
    res["tables_equal"] = all(s["tables_equal"] for s in res["step"].values())
    res["walk_kernels_no_slower"] = all(w["branch_median_not_above_parent_slowest"] for s in res["step"].values() for w in s["walk_kernels"].values())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
