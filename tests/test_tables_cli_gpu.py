"""The seven analysis tables of `vgaligner map` (rs-vgaligner_amd/host/vgh_tables.cpp) all at once, and on a device slot that gets
no read: --coverage, --path-support, --pileup, --genotype, --genotype-likelihood, --path-edit and --call-variants together on one
context, the same over `--devices 0,0,0 --chunk-reads 1` with two reads (the middle slot stays empty), with and without the fast
exit, and each switch alone.  Every comparison is byte equality of the files the runs write."""
import os
import subprocess

import pytest

from helpers import DATA, ROOT, pkg

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
SWITCHES = {
    "coverage": ["--coverage"],
    "path-support": ["--path-support"],
    "pileup": ["--pileup"],
    "genotype": ["--genotype"],
    "genotype-likelihood": ["--genotype-likelihood"],
    "path-edit": ["--path-edit"],
    "call-variants": ["--call-variants", "--call-min-depth", "1", "--call-min-qual", "0"],
}
# the line of each analysis in the driver's summary on stderr
SUMMARY = ("[vgaligner] Coverage:", "[vgaligner] Path support:", "[vgaligner] genotype:", "[vgaligner] genotype-likelihood:", "[vgaligner] path-edit:",
           "[vgaligner] Pileup:", "[vgaligner] call-variants:")
GAF = {"-chains.gaf", "-alignments.gaf"}


def two_reads_of_equal_length(p):
    reads = p.readsim.config3_reads(DRB1, 200, 2000)
    first = {}
    for r in reads:
        if len(r.seq) in first:
            return [first[len(r.seq)], r]
        first[len(r.seq)] = r
    raise AssertionError("no two simulated reads of one length")


def test_cli(tmp_path):
    p = pkg()
    d = str(tmp_path)
    reads = two_reads_of_equal_length(p)
    # three slots, two reads of one length: the first read, nothing, the second read (vgh::plan_shards)
    assert p.hostlib.plan_shards([len(r.seq) for r in reads], 3, 1) == [(0, 1, 0), (1, 2, 2)]
    fa = os.path.join(d, "r.fa")
    p.readsim.write_fasta(reads, fa)

    def run(args, env=None):
        # one process after the other, each under its own time limit; the first that fails (a signal and a time-out included) ends the test
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=300, env=None if env is None else dict(os.environ, **env))
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "-D", "-G", DRB1]
    everything = [f for flags in SWITCHES.values() for f in flags]
    three_slots = ["--devices", "0,0,0", "--chunk-reads", "1"]
    err = {}
    err["all"] = run(common + ["-o", os.path.join(d, "all")] + everything).stderr
    err["three"] = run(common + ["-o", os.path.join(d, "three")] + everything + three_slots).stderr
    err["slow"] = run(common + ["-o", os.path.join(d, "slow")] + everything + three_slots, env={"VGA_NO_FAST_EXIT": "1"}).stderr
    alone = {name: "alone%d" % i for i, name in enumerate(SWITCHES)}  # (no output prefix is the beginning of another)
    for name, flags in SWITCHES.items():
        run(common + ["-o", os.path.join(d, alone[name])] + flags)

    def files(out):  # suffix -> bytes
        return {f[len(out):]: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.startswith(out + "-") and f.endswith((".tsv", ".gaf"))}

    want = files("all")
    assert GAF < set(want) and len(want) == 13, sorted(want)  # (3 + 2 + 1 + 1 + 1 + 2 + 1 tables)
    assert "1 GPU context(s), 1 batch(es)" in err["all"], err["all"]
    for out in ("three", "slow"):
        assert "3 GPU context(s), 2 batch(es)" in err[out], err[out]
        got = files(out)
        assert set(got) == set(want), (out, sorted(got))
        for suffix in want:
            assert got[suffix] == want[suffix], (out, suffix)
    # every table is what the switch that owns it writes alone, and no run writes a table of its own
    union = set()
    for name in SWITCHES:
        tables = {s: t for s, t in files(alone[name]).items() if s not in GAF}
        assert tables and not (set(tables) & union), (name, sorted(tables))
        union |= set(tables)
        for suffix, text in tables.items():
            assert want.get(suffix) == text, (name, suffix)
    assert union | GAF == set(want), sorted(union)
    # the summary of the seven analyses: one line each, the same over three slots
    lines = {out: [ln for ln in err[out].splitlines() if ln.startswith(SUMMARY)] for out in ("all", "three")}
    assert len(lines["all"]) == 7 and lines["three"] == lines["all"], lines
