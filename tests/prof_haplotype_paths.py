"""diagnostic: what keeping the deficit store and summing it by (set, haplotype) costs.  One JSON object on
stdout (profiles/haplotype_paths.json).  Every measurement runs in a child process of its own with a time limit of its own, and the
sides of a comparison alternate, so that both see the same box in the same minutes; the first child that fails ends the script.
`--parent-lib` names a libvga_hip.so built from the parent commit by the same compiler (the binding's VGA_LIB).

  bench_ab   the switch off costs nothing: `python bench.py --gpus 1 --steps 3 --warmup 1` (config 3) with this tree's library and
             with the parent's, alternating, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  step       one process: config 3 steps (10 000 x 10 kbp reads: map + align) with the pileup counted, path support scored and the
             phase store kept, without and with the deficit store, alternating: reads/s of each step and k_hp_keep's time in it (the
             first step with the store on pays its growth); then the variants called, their heterozygous sites linked and chained,
             and vga_haplotype_paths three times: the wall time of the whole call and its kernels, beside vga_phase_tags and
             vga_phase_set_links on the same store.
  seam       vga_haplotype_paths_lists on the synthetic lists of tests/prof_phase_join.py (`--reads` reads of 10 kbp) for 16 and
             1 024 sites under the sets of the chain on their links, with 12, 256 and 4 096 paths of random deficit bytes.

    python tests/prof_haplotype_paths.py --parent-lib PATH [--parts bench_ab,step,seam] [--repeats 3] [--reads 10000] [--steps 4]
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
SEAM_SITES = (16, 1024)
SEAM_PATHS = (12, 256, 4096)
CHILD_LIMIT = {"bench": 600, "step": 600, "seam": 600}


def kernel_ms(ctx, prefixes=("k_ph", "k_hc", "k_sj", "k_hp")):
    return {t["name"]: {"ms": round(t["ms"], 4), "launches": t["launches"]} for t in ctx.kernel_times() if t["name"].startswith(prefixes)}


def timed(ctx, call, repeats=3):
    """the call once to warm up, then `repeats` times: wall time and the kernels of each -> (last result, runs)"""
    got = call()
    runs = []
    for _ in range(repeats):
        t1 = time.perf_counter()
        got = call()
        runs.append({"call_wall_ms": round((time.perf_counter() - t1) * 1e3, 2), "kernels": kernel_ms(ctx)})
    return got, runs


def child_step(n_reads, steps, warmup):
    import numpy as np

    import __graft_entry__ as ge
    import path_support_ref

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(DRB1, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(DRB1, n_reads)])
    _, paths = path_support_ref.parse_gfa(DRB1)
    ctx.path_support_begin(*path_support_ref.packed_steps(paths))
    ctx.pileup_begin()
    for _ in range(warmup):
        b.map_align_raw()
    ctx.phase_begin()

    def step():
        t1 = time.perf_counter()
        b.map_align_raw()
        ctx.synchronize()
        dt = time.perf_counter() - t1
        keep = [t for t in ctx.kernel_times() if t["name"] == "k_hp_keep"]
        return {"reads_per_s": round(n_reads / dt, 1), "k_hp_keep_busy_ms": round(keep[0]["busy_ms"], 4) if keep else None}

    # without and with the deficit store, alternating; the phase store is emptied between the sides so that both keep as much
    sides = {"phase_store_only": [], "with_deficit_store": []}
    for _ in range(steps):
        ctx.phase_reset()
        sides["phase_store_only"].append(step())
        ctx.phase_reset()
        ctx.haplotype_paths_begin()
        sides["with_deficit_store"].append(step())   # (a fresh store each time: every one of these steps pays the growth)
        ctx.haplotype_paths_end()
    ctx.pileup_reset()
    ctx.phase_reset()
    ctx.haplotype_paths_begin()
    grown = []
    for _ in range(steps):
        grown.append(step())                          # (the store doubles as it fills: the later steps grow less often)
    ctx.synchronize()
    calls = ctx.variant_call()
    het = calls["x"] < calls["y"]
    pos, x, y = calls["pos"][het], calls["x"][het], calls["y"][het]
    links, sr, n = ctx.phase_links(pos, x, y)
    ps, flip, link_d = p.binding.phase_chain(links)
    tags = ctx.phase_tags(pos, x, y, ps, flip)[0]
    _, tag_runs = timed(ctx, lambda: ctx.phase_tags(pos, x, y, ps, flip, cap=len(tags)))
    _, link_runs = timed(ctx, lambda: ctx.phase_set_links(pos, x, y, ps, flip))
    (reads, table, n_sets, n), runs = timed(ctx, lambda: ctx.haplotype_paths(pos, x, y, ps, flip))
    d, sc = ctx.haplotype_paths_store()
    out = {"reads_kept": int(n), "paths": int(d.shape[1]), "store_bytes": int(d.size + sc.size), "reads_scored": int(sc.sum()), "heterozygous_sites": int(len(pos)),
           "sets": int(n_sets), "groups_with_reads": int((reads > 0).sum()), "steps_alternating": sides, "steps_filling_one_store": grown,
           "vga_phase_tags_with_room": tag_runs, "vga_phase_set_links": link_runs, "vga_haplotype_paths": runs}
    print(json.dumps(out), flush=True)


def child_seam(n_reads):
    """one process: the synthetic lists of prof_phase_join.py (n_reads reads of 10 kbp on a graph of 2^18 bases), the same lists for
    every shape"""
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    ctx = p.Context(0)
    rng = np.random.default_rng(1)
    n_bases, length, n_sparse = 1 << 18, 10000, 1000
    recs, words, at = np.zeros((n_reads, 3), dtype=np.uint32), [], 0
    for r in range(n_reads):
        start = int(rng.integers(0, n_bases - length))
        sp = start + np.unique(rng.integers(1, length - 1, size=n_sparse))
        edges = np.concatenate([[start], sp + 1])
        ends = np.concatenate([sp, [start + length]])
        keep = ends > edges
        ev = np.stack([edges[keep] << 1, (ends[keep] << 1) | 1], axis=1).reshape(-1)
        sparse = (sp << 3) | rng.integers(0, 7, size=len(sp))
        recs[r] = (at, len(ev), len(sparse))
        words.append(ev.astype(np.uint32))
        words.append(sparse.astype(np.uint32))
        at += len(ev) + len(sparse)
    words = np.concatenate(words)
    out = {"reads": n_reads, "graph_bases": n_bases, "shapes": {}}
    for n_sites in SEAM_SITES:
        pos = np.sort(rng.choice(n_bases, size=n_sites, replace=False)).astype(np.uint32)
        x = rng.integers(0, 4, size=n_sites).astype(np.uint8)
        y = (x + 1 + rng.integers(0, 4 - x)).astype(np.uint8)
        ref = np.where(rng.integers(0, 2, size=n_sites) == 0, x, np.minimum(y, 3)).astype(np.uint8)
        links, _ = ctx.phase_links_lists(recs, words, n_bases, pos, x, y, ref)
        ps, flip, link_d = p.binding.phase_chain(links)
        for n_paths in SEAM_PATHS:
            d = rng.integers(0, 65, size=(n_reads, n_paths)).astype(np.uint8)
            sc = np.ones(n_reads, dtype=np.uint8)
            entry = {"sites": n_sites, "paths": n_paths, "sets": int((link_d == 0).sum())}
            try:
                (reads, table, n_sets), runs = timed(ctx, lambda: ctx.haplotype_paths_lists(recs, words, n_bases, d, sc, pos, x, y, ref, ps, flip))
                entry.update(tagged_scored_reads=int(reads.sum()), table_bytes=int(table.nbytes), runs=runs)
            except p.VgaError as e:
                entry["refused"] = "%d: %s" % (e.code, e)
            out["shapes"]["%d sites, %d paths" % (n_sites, n_paths)] = entry
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
    ap.add_argument("--parts", default="bench_ab,step,seam")
    ap.add_argument("--repeats", type=int, default=3)
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
    out = {"what": "what the deficit store and the sums of the haplotype paths cost on one MI355X (DESIGN.md section 29); no figure here is asserted by a test"}
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
    if "step" in parts:
        out["step"] = dict(run_child([me, "--child", str(a.reads), str(a.steps), str(a.warmup)], env=env, limit=CHILD_LIMIT["step"]),
                           workload="config 3: %d reads of 10 kbp on DRB1-3123, path support scored, the pileup counted, the phase store kept" % a.reads)
    if "seam" in parts:
        out["seam"] = run_child([me, "--child", "seam", str(a.reads)], env=env, limit=CHILD_LIMIT["seam"])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
