"""diagnostic: what counting the set links costs.  One JSON object on stdout (profiles/phase_join.json).
Every measurement runs in a child process of its own with a time limit of its own, and the sides of a comparison alternate, so that
both see the same box in the same minutes; the first child that fails ends the script.  `--parent-lib` names a libvga_hip.so built
from the parent commit by the same compiler (the binding's VGA_LIB).

  bench_ab   the switch off costs nothing: `python bench.py --gpus 1 --steps 3 --warmup 1` (config 3) with this tree's library and
             with the parent's, alternating, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  step       one process: config 3 steps (10 000 x 10 kbp reads: map + align) with the pileup counted and the phase store kept,
             then the variants called, their heterozygous sites linked and chained, and vga_phase_set_links three times: the wall
             time of the whole call and the time of k_ph_obs, k_hc_tags, k_sj_bits and k_sj_pairs in it, beside vga_phase_tags on
             the same store; the same once more with every site its own set as far as PJ_MAX_SETS allows (the first 4096 sites).
  seam       vga_phase_set_links_lists on the synthetic lists of tests/prof_haplotag.py (`--reads` reads of 10 kbp with a tenth of
             their bases in sparse words) for 16, 1 024 and 65 536 sites under the sets of the chain on their links; a site count
             whose chain has more than 4096 sets is halved until it has not, and the entry says so.

    python tests/prof_phase_join.py --parent-lib PATH [--parts bench_ab,step,seam] [--repeats 3] [--reads 10000] [--steps 4]
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
SEAM_SITES = (16, 1024, 65536)
CHILD_LIMIT = {"bench": 600, "step": 600, "seam": 600}


def kernel_ms(ctx):
    return {t["name"]: {"ms": round(t["ms"], 4), "launches": t["launches"]} for t in ctx.kernel_times() if t["name"].startswith(("k_ph", "k_hc", "k_sj"))}


def timed(ctx, call, repeats=3):
    """the call once to warm up, then `repeats` times: wall time and the kernels of each -> (last result, runs)"""
    got = call()
    runs = []
    for _ in range(repeats):
        t1 = time.perf_counter()
        got = call()
        runs.append({"call_wall_ms": round((time.perf_counter() - t1) * 1e3, 2), "kernels": kernel_ms(ctx)})
    return got, runs


def join_summary(p, table, n_sets):
    t1 = time.perf_counter()
    root, flip, joins, agree, conflict = p.binding.phase_join(table, n_sets)
    return {"sets": int(n_sets), "pairs_with_a_read": int((table.sum(axis=1) > 0).sum()), "joins": int(len(joins)), "agreeing": agree, "conflicting": conflict,
            "vga_phase_join_host_ms": round((time.perf_counter() - t1) * 1e3, 2)}


def child_step(n_reads, steps, warmup):
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(DRB1, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(DRB1, n_reads)])
    ctx.pileup_begin()
    for _ in range(warmup):
        b.map_align_raw()
    ctx.phase_begin()
    for _ in range(steps):
        b.map_align_raw()
    ctx.synchronize()
    calls = ctx.variant_call()
    het = calls["x"] < calls["y"]
    pos, x, y = calls["pos"][het], calls["x"][het], calls["y"][het]
    links, sr, n = ctx.phase_links(pos, x, y)
    ps, flip, link_d = p.binding.phase_chain(links)
    tags = ctx.phase_tags(pos, x, y, ps, flip)[0]
    (_, _), tag_runs = timed(ctx, lambda: ctx.phase_tags(pos, x, y, ps, flip, cap=len(tags)))
    (table, n_sets, n), runs = timed(ctx, lambda: ctx.phase_set_links(pos, x, y, ps, flip))
    out = {"reads_kept": int(n), "calls": int(len(calls["pos"])), "heterozygous_sites": int(len(pos)), "chain": join_summary(p, table, n_sets),
           "vga_phase_tags_with_room": tag_runs, "vga_phase_set_links": runs}
    # every site its own set, the first PJ_MAX_SETS sites: the most sets one call serves, on the real store
    m = min(len(pos), p.binding.PHASE_JOIN_MAX_SETS)
    own, none = np.arange(1, m + 1, dtype=np.uint32), np.zeros(m, dtype=np.uint8)
    (table, n_sets, n), runs = timed(ctx, lambda: ctx.phase_set_links(pos[:m], x[:m], y[:m], own, none))
    out["every_site_its_own_set"] = dict(join_summary(p, table, n_sets), sites=int(m), vga_phase_set_links=runs)
    print(json.dumps(out), flush=True)


def child_seam(n_reads):
    """one process: the synthetic lists of prof_haplotag.py (n_reads reads of 10 kbp on a graph of 2^18 bases), the same lists for
    every site count"""
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
    out = {"reads": n_reads, "graph_bases": n_bases, "words_per_read": round(len(words) / n_reads, 1), "sites": {}}
    for asked in SEAM_SITES:
        n_sites, halved = asked, []
        while True:
            pos = np.sort(rng.choice(n_bases, size=n_sites, replace=False)).astype(np.uint32)
            x = rng.integers(0, 4, size=n_sites).astype(np.uint8)
            y = (x + 1 + rng.integers(0, 4 - x)).astype(np.uint8)
            ref = np.where(rng.integers(0, 2, size=n_sites) == 0, x, np.minimum(y, 3)).astype(np.uint8)
            links, _ = ctx.phase_links_lists(recs, words, n_bases, pos, x, y, ref)
            ps, flip, link_d = p.binding.phase_chain(links)
            sets = int((link_d == 0).sum())
            if sets <= p.binding.PHASE_JOIN_MAX_SETS or n_sites <= 16:
                break
            halved.append({"sites": n_sites, "sets": sets})
            n_sites //= 2
        entry = {"sites_asked": asked, "sites": n_sites, "more_than_4096_sets_at": halved, "sets": sets}
        try:
            tags = ctx.phase_tags_lists(recs, words, n_bases, pos, x, y, ref, ps, flip)
            _, tag_runs = timed(ctx, lambda: ctx.phase_tags_lists(recs, words, n_bases, pos, x, y, ref, ps, flip, cap=len(tags)))
            (table, n_sets, _), runs = timed(ctx, lambda: ctx.phase_set_links_lists(recs, words, n_bases, pos, x, y, ref, ps, flip))
            entry.update(join_summary(p, table, n_sets), vga_phase_tags_lists_with_room=tag_runs, runs=runs)
        except p.VgaError as e:
            entry["refused"] = "%d: %s" % (e.code, e)
        out["sites"][str(asked)] = entry
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
    out = {"what": "what counting the set links of the phase join costs on one MI355X (DESIGN.md section 28); no figure here is asserted by a test"}
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
                           workload="config 3: %d reads of 10 kbp on DRB1-3123, the phase store kept over %d steps after %d, the pileup counted" %
                           (a.reads, a.steps, a.warmup))
    if "seam" in parts:
        out["seam"] = run_child([me, "--child", "seam", str(a.reads)], env=env, limit=CHILD_LIMIT["seam"])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
