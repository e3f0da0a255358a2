"""The phase join, the parts that need no GPU: the join rule of csrc/vga_phase_join.hpp compiled alone with a host compiler, against
the reference (tests/phase_join_ref.py), against vga_phase_join of the built library and against cases written out by hand; the
reference's table by hand; the calls in the ABI; the command line's refusals and usage text; the planted sample on the oracle's
alignments GAF; and the scratch budget of the two kernels from a cross-compile for gfx950.  Without the feature every test here stops
at the missing header, the missing binding call or symbols, the unknown switch or the missing kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

import phase_cases as P
import phase_join_ref as ref
import phase_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_phase_set_links", "vga_phase_set_links_lists", "vga_phase_join"]

# reads cases from the standard input until it ends: "S min_reads H", the S (S + 1) / 2 rows, then ps and flip of the H sites;
# prints set_root | set_flip | joins | n_joins n_agree n_conflict | ps' | flip'
HARNESS = r"""
#include "vga_phase_join.hpp"
#include <cstdio>
int main()
{
    unsigned long long S, m, H;
    while (scanf("%llu %llu %llu", &S, &m, &H) == 3) {
        std::vector<uint32_t> table(vga_pair_count(S) * PJ_COLS + 1), ps(H + 1), root(S + 1), joins((S + 1) * PJ_JOIN_COLS), ps2(H + 1);
        std::vector<uint8_t> flip(H + 1), sflip(S + 1), flip2(H + 1);
        for (size_t i = 0; i < vga_pair_count(S) * PJ_COLS; i++) { unsigned v; if (scanf("%u", &v) != 1) return 2; table[i] = v; }
        for (size_t h = 0; h < H; h++) { unsigned v; if (scanf("%u", &v) != 1) return 2; ps[h] = v; }
        for (size_t h = 0; h < H; h++) { unsigned v; if (scanf("%u", &v) != 1) return 2; flip[h] = (uint8_t)v; }
        uint64_t nj = 0, na = 0, nc = 0;
        pj_join(S, table.data(), (uint32_t)m, root.data(), sflip.data(), joins.data(), &nj, &na, &nc);
        const uint64_t sets = pj_sites(H, ps.data(), flip.data(), root.data(), sflip.data(), ps2.data(), flip2.data());
        if (H && sets != S) return 3;
        for (size_t s = 0; s < S; s++) printf(" %u", root[s]);
        printf(" |");
        for (size_t s = 0; s < S; s++) printf(" %u", sflip[s]);
        printf(" |");
        for (size_t k = 0; k < nj * PJ_JOIN_COLS; k++) printf(" %u", joins[k]);
        printf(" | %llu %llu %llu |", (unsigned long long)nj, (unsigned long long)na, (unsigned long long)nc);
        for (size_t h = 0; h < H; h++) printf(" %u", ps2[h]);
        printf(" |");
        for (size_t h = 0; h < H; h++) printf(" %u", flip2[h]);
        printf("\n");
    }
    return 0;
}
"""


def binding():
    b = pkg().binding
    assert hasattr(b, "phase_join"), "the binding has no phase join"
    return b


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """csrc/vga_phase_join.hpp alone, with g++ and every warning an error"""
    d = tmp_path_factory.mktemp("pj")
    src = d / "pj.cpp"
    src.write_text(HARNESS)
    assert os.path.exists(os.path.join(CSRC, "vga_phase_join.hpp")), "no csrc/vga_phase_join.hpp"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(d / "pj")])

    def run(cases):
        """cases: [(S, table rows, min_reads, ps, flip)] -> [(root, flip, joins, agree, conflict, ps', flip')]"""
        text = ""
        for S, rows, m, ps, flip in cases:
            text += "%d %d %d\n%s\n%s\n%s\n" % (S, m, len(ps), " ".join(str(int(v)) for r in rows for v in r), " ".join(str(int(p)) for p in ps),
                                               " ".join(str(int(f)) for f in flip))
        out = subprocess.run([str(d / "pj")], input=text, capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        got = []
        for line in out:
            f = [[int(v) for v in part.split()] for part in line.split("|")]
            joins = [tuple(f[2][k:k + 4]) for k in range(0, len(f[2]), 4)]
            assert f[3][0] == len(joins)
            got.append((f[0], f[1], joins, f[3][1], f[3][2], f[4], f[5]))
        return got

    return run


def make(S, pairs):
    """the table of S sets with the given rows {(s, t): (aa, ab, ba, bb)}, everything else 0"""
    t = np.zeros((S * (S + 1) // 2, 4), dtype=np.uint32)
    for (s, u), n in pairs.items():
        t[ref.pair_index(S, s, u)] = n
    return t


def own(S):
    """S sites, every one its own set"""
    return list(range(1, S + 1)), [0] * S


# (name, S, rows, min_reads) -> (set_root, set_flip, joins, agreeing, conflicting)
HAND = [
    # 0 - 1 by 5 reads cis, 1 - 2 by 4 cis; the weakest link says 0 - 2 trans: it closes the triangle against what is implied
    ("triangle", 3, {(0, 1): (5, 0, 0, 0), (1, 2): (1, 0, 0, 3), (0, 2): (0, 2, 1, 0)}, 2, ([0, 0, 0], [0, 0, 0], [(0, 1, 5, 0), (1, 2, 4, 0)], 0, 1)),
    # two trans links make a cis relation, and the third link agrees with it
    ("trans twice", 3, {(0, 1): (0, 5, 0, 0), (1, 2): (0, 1, 3, 0), (0, 2): (3, 0, 0, 0)}, 2, ([0, 0, 0], [0, 1, 0], [(0, 1, 0, 5), (1, 2, 0, 4)], 1, 0)),
    # three links of the same diff: (0, 1), (0, 2), (1, 2) in that order, so (1, 2) is the one that conflicts and set 2 is flipped
    ("ties", 3, {(0, 1): (3, 0, 0, 0), (0, 2): (0, 3, 0, 0), (1, 2): (0, 0, 0, 3)}, 2, ([0, 0, 0], [0, 0, 1], [(0, 1, 3, 0), (0, 2, 0, 3)], 0, 1)),
    # a tie in diff between (0, 3) and (1, 2) with a larger cis on the later pair: (s, t) decides, not cis
    ("ties by s", 4, {(1, 2): (9, 3, 3, 0), (0, 3): (0, 2, 2, 1)}, 3, ([0, 1, 1, 0], [0, 0, 0, 1], [(0, 3, 1, 4), (1, 2, 9, 6)], 0, 0)),
    ("at min_reads", 2, {(0, 1): (3, 1, 1, 2)}, 3, ([0, 0], [0, 0], [(0, 1, 5, 2)], 0, 0)),
    ("below min_reads", 2, {(0, 1): (3, 1, 1, 2)}, 4, ([0, 1], [0, 0], [], 0, 0)),
    ("cis = trans", 2, {(0, 1): (1, 2, 0, 1)}, 1, ([0, 1], [0, 0], [], 0, 0)),
    ("one read", 2, {(0, 1): (0, 0, 1, 0)}, 1, ([0, 0], [0, 1], [(0, 1, 0, 1)], 0, 0)),
    # 1 - 2 are joined first (trans), then 0 reaches them through 2 (trans): 0 names the set and keeps its orientation, so 2 is
    # flipped against it and 1, trans to 2, is not
    ("smallest last", 3, {(1, 2): (0, 9, 0, 0), (0, 2): (0, 0, 4, 0)}, 2, ([0, 0, 0], [0, 0, 1], [(1, 2, 0, 9), (0, 2, 0, 4)], 0, 0)),
    # the diagonal is no link, however large
    ("diagonal", 2, {(0, 0): (50, 0, 0, 7), (1, 1): (9, 0, 0, 60)}, 1, ([0, 1], [0, 0], [], 0, 0)),
    ("no set", 0, {}, 2, ([], [], [], 0, 0)),
    ("one set", 1, {(0, 0): (4, 0, 0, 5)}, 2, ([0], [0], [], 0, 0)),
]


def test_join_rule_by_hand(harness):
    b = binding()
    cases = [(S, make(S, pairs), m) + own(S) for _, S, pairs, m, _ in HAND]
    got = harness(cases)
    for (name, S, pairs, m, want), g in zip(HAND, got):
        assert g[:5] == want, (name, g)
        assert ref.join(make(S, pairs), S, m) == want, name
        root, flip, joins, agree, conflict = b.phase_join(make(S, pairs), S, m)
        assert (root.tolist(), flip.tolist(), [tuple(j) for j in joins.tolist()], agree, conflict) == want, name
        assert root.dtype == np.uint32 and flip.dtype == np.uint8 and joins.dtype == np.uint32 and joins.shape == (len(want[2]), 4)


def test_join_rule_equals_the_reference(harness):
    b = binding()
    rng = np.random.default_rng(17)
    cases = []
    for k in range(60):
        S = int(rng.integers(0, 13))
        t = rng.integers(0, 4, size=(S * (S + 1) // 2, 4)) * rng.integers(0, 2, size=(S * (S + 1) // 2, 1))   # small counts: many ties
        m = int(rng.integers(1, 4))
        # the sites: every set opened in order, then more sites that join an earlier set
        ps = []
        for s in range(S):
            ps.append(len(ps) + 1)
            while rng.integers(0, 3) == 0:
                ps.append(ps[int(rng.integers(0, len(ps)))])
        flip = [int(v) for v in rng.integers(0, 2, size=len(ps))]
        cases.append((S, t.astype(np.uint32), m, ps, flip))
    joined = 0
    for (S, t, m, ps, flip), g in zip(cases, harness(cases)):
        want = ref.join(t, S, m)
        assert g[:5] == want, (S, m, t.tolist())
        root, sflip, joins, agree, conflict = b.phase_join(t, S, m)
        assert (root.tolist(), sflip.tolist(), [tuple(j) for j in joins.tolist()], agree, conflict) == want
        ps2, flip2 = ref.sites(ps, flip, want[0], want[1])
        assert (g[5], g[6]) == (ps2, flip2)
        # what ph_check_sets demands of the joined sets, and what a join is
        assert ref.check_sets(ps) and ref.check_sets(ps2) and all(q <= p for p, q in zip(ps, ps2))
        assert len(set(ps2)) == S - len(want[2]) and all(f in (0, 1) for f in flip2)
        joined += len(want[2])
    assert joined > 50
    for bad in (0, 65536):
        with pytest.raises(pkg().VgaError):
            b.phase_join(make(2, {}), 2, bad)
    with pytest.raises(pkg().VgaError):
        b.phase_join(make(2, {}), 3, 2)
    assert b.phase_join(make(2, {(0, 1): (0, 65535, 0, 0)}), 2, 65535)[2].tolist() == [[0, 1, 0, 65535]]


def test_joined_sites_by_hand(harness):
    binding()
    # sets 1 = sites 0, 2; 2 = sites 1, 4; 4 = site 3, under "smallest last": everything lands in set 1, set 4 (index 2) flipped
    name, S, pairs, m, want = HAND[8]
    ps, flip = [1, 2, 1, 4, 2], [0, 0, 1, 0, 1]
    g = harness([(S, make(S, pairs), m, ps, flip)])[0]
    assert (g[5], g[6]) == ([1, 1, 1, 1, 1], [0, 0, 1, 1, 1]) == ref.sites(ps, flip, want[0], want[1])
    # nothing joined: the chain's own
    g = harness([(3, make(3, {}), 2, ps, flip)])[0]
    assert (g[5], g[6]) == (ps, flip)


def test_reference_table_by_hand():
    binding()
    # TINY_OBS, two sites in one set, site 1 flipped: read 0 votes a twice (x, and y flipped), reads 1 and 2 once a and once b (a
    # tie: no tag), read 3 shows "other" at site 0 and y flipped at site 1: a
    obs = P.TINY_OBS
    assert ref.tags(obs, [1, 1], [0, 1]) == [{0: 0}, {}, {}, {0: 0}, {}, {}]
    assert ref.table(obs, [1, 1], [0, 1]).tolist() == [[2, 0, 0, 0]]
    # each site its own set: votes are the observations; read 3 shows "other" at site 0 and is tagged in set 1 alone
    assert ref.tags(obs, [1, 2], [0, 0]) == [{0: 0, 1: 1}, {0: 1, 1: 1}, {0: 0, 1: 0}, {1: 1}, {}, {}]
    assert ref.table(obs, [1, 2], [0, 0]).tolist() == [[2, 0, 0, 1], [1, 1, 0, 1], [1, 0, 0, 3]]
    # EDGE_OBS, interleaved sets: set 1 = sites 0, 2, 4 (site 4 flipped), set 2 = sites 1, 3
    ps, flip = [1, 2, 1, 2, 1], [0, 0, 0, 0, 1]
    # read 0: set 1 votes a (site 0), a (site 4: y flipped) -> a; set 2: a (site 1) -> a.  read 1: a | b.  read 2: a (site 2) | a.
    # read 3: site 2 shows y -> b | sites 1, 3: x and y: a tie.  read 5: site 0 a, site 4 y flipped a -> a | site 3 a.
    assert ref.tags(P.EDGE_OBS, ps, flip) == [{0: 0, 1: 0}, {0: 0, 1: 1}, {0: 0, 1: 0}, {0: 1}, {}, {0: 0, 1: 0}]
    t = ref.table(P.EDGE_OBS, ps, flip)
    assert t.dtype == np.uint32 and t.tolist() == [[4, 0, 0, 1], [3, 1, 0, 0], [3, 0, 0, 1]]
    assert ref.join(t, 2, 2) == ([0, 0], [0, 0], [(0, 1, 3, 1)], 0, 0) and ref.join(t, 2, 3) == ([0, 1], [0, 0], [], 0, 0)
    assert ref.table([], ps, flip).shape == (0, 4)
    assert ref.sets_tsv(ps, t, [0, 0], [0, 0]) == ref.SETS_HEADER + "\n1\t3\t4\t1\t1\t0\n2\t2\t3\t1\t1\t0\n"
    assert ref.joins_tsv(ps, [(0, 1, 3, 1)]) == ref.JOINS_HEADER + "\n1\t2\t3\t1\tcis\n"


# ---- the ABI
def test_abi_lists_and_exports_the_calls(tmp_path):
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert getattr(L, name) is not None and getattr(L, name).argtypes is not None
    src = tmp_path / "pj.c"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*c)(vga_ctx *, uint64_t, const uint32_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint8_t *, uint64_t, uint32_t *,\n"
                   "         uint64_t *, uint64_t *) = vga_phase_set_links;\n"
                   "int (*l)(vga_ctx *, uint64_t, uint64_t, const uint32_t *, uint64_t, const uint32_t *, uint64_t, const uint32_t *, const uint8_t *,\n"
                   "         const uint8_t *, const uint8_t *, const uint32_t *, const uint8_t *, uint64_t, uint32_t *, uint64_t *) = vga_phase_set_links_lists;\n"
                   "int (*j)(uint64_t, const uint32_t *, uint32_t, uint32_t *, uint8_t *, uint32_t *, uint64_t *, uint64_t *, uint64_t *) = vga_phase_join;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "pj.o")])
    hpp = open(os.path.join(CSRC, "vga_phase_join.hpp")).read()
    b = p.binding
    assert b.PHASE_JOIN_COLS == 4 == int(re.search(r"#define PJ_COLS (\d+)u", hpp).group(1))
    assert b.PHASE_JOIN_MAX_SETS == 4096 == int(re.search(r"#define PJ_MAX_SETS (\d+)u", hpp).group(1))
    assert b.PHASE_JOIN_TILE == int(re.search(r"#define PJ_TILE (\d+)u", hpp).group(1))
    assert b.PHASE_JOIN_MIN_READS == 2 == int(re.search(r"#define PJ_MIN_READS_DEFAULT (\d+)u", hpp).group(1))
    assert b.PHASE_JOIN_MAX_MIN_READS == 65535 == int(re.search(r"#define PJ_MIN_READS_MAX (\d+)u", hpp).group(1))
    for name in ("phase_set_links", "phase_set_links_lists"):
        assert hasattr(b.Context, name), name


def test_null_context_return_codes():
    L = pkg().binding.load_library()
    assert L.vga_phase_set_links(None, 0, None, None, None, None, None, 0, None, None, None) == -1
    assert L.vga_phase_set_links_lists(None, 0, 0, None, 0, None, 0, None, None, None, None, None, None, 0, None, None) == -1
    assert L.vga_phase_join(0, None, 2, None, None, None, None, None, None) == -1
    assert L.vga_phase_join(0, None, 0, None, None, None, None, None, None) == -1


# ---- the command line: the refusals before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE, "map", "-i", str(cwd / "none"), "-f", str(cwd / "none.fa"), "-p", "abpoa"] + args, cwd=str(cwd), capture_output=True,
                          text=True, timeout=300, env=env)


def test_cli_argument_errors(tmp_path):
    pkg()
    phase = ["--call-variants", "--phase"]
    for args, words in ((["--call-variants", "--phase-join"], ("--phase-join", "--phase")), (["--phase-join"], ("--phase-join", "--phase")),
                        (phase + ["--phase-join-min-reads", "3"], ("--phase-join-min-reads", "--phase-join")),
                        (phase + ["--phase-join", "--phase-join-min-reads", "0"], ("--phase-join-min-reads", "1 to 65535")),
                        (phase + ["--phase-join", "--phase-join-min-reads", "65536"], ("--phase-join-min-reads", "1 to 65535")),
                        (phase + ["--phase-join", "--phase-join-min-reads", "2x"], ("--phase-join-min-reads", "1 to 65535"))):
        pr = run_cli(["-D", "-G", "none.gfa"] + args, tmp_path)
        assert pr.returncode != 0 and all(w in pr.stderr for w in words), (args, pr.stderr)
        assert pr.stderr.strip().count("\n") == 0 and "device" not in pr.stderr.lower() and "hip" not in pr.stderr.lower(), pr.stderr
        assert not os.listdir(str(tmp_path))
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "[--phase-join [--phase-join-min-reads 2]]" in usage.stderr, usage.stderr


# ---- the planted sample on the oracle's text
def test_planted_sets_are_joined(oracle):
    """The planted sample of tests/phase_cases.py (haplotype A carries substitutions at s1 and s3, B at s2; 12 reads of 1000 bases
    each).  With --phase-min-links 65535 the chain joins nothing and every site is its own set; the join then brings the three planted
    sites into one set, their letters arranged as the default chain arranges them.  On the default chain the join leaves fewer sets,
    the planted one among them as it was."""
    binding()
    rs = pkg().readsim
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    a = oracle_index_arrays(ix)
    reads, at, new, old = P.planted_sample(rs, DRB1, a["node_seq_idx"])
    _, ag, _ = oracle.map_reads(ix, [n for n, _ in reads], [s for _, s in reads])
    chain = ref.gaf(ag, a["node_seq_idx"], a["seq_fwd"])
    alone = ref.gaf(ag, a["node_seq_idx"], a["seq_fwd"], min_links=65535)
    for name, g in (("default chain", chain), ("every site alone", alone)):
        print(name, "S", g["n_sets"], "joins", len(g["joins"]), "agreeing", g["agree"], "conflicting", g["conflict"])
        assert ref.check_sets(g["ps2"]) and len(set(g["ps2"])) == g["n_sets"] - len(g["joins"])
    assert alone["pos"] == chain["pos"] and alone["ps"] == list(range(1, len(alone["pos"]) + 1)) and not any(alone["flip"])
    h = [chain["pos"].index(p) for p in at]
    assert len({chain["ps"][k] for k in h}) == 1, "the default chain holds the planted sites in one set"
    # every site its own set: the three planted sites land in one joined set ...
    assert len({alone["ps2"][k] for k in h}) == 1 and len(alone["joins"]) >= 2
    # ... with the letters of haplotype a (flip ? y : x) arranged as the default chain arranges them, up to the swap of a and b
    letters = lambda g, flips: ["ACGT-"[g["y"][k] if flips[k] else g["x"][k]] for k in h]
    want, got = letters(chain, chain["flip"]), letters(alone, alone["flip2"])
    other = ["ACGT-"[chain["x"][k] if chain["flip"][k] else chain["y"][k]] for k in h]
    assert got in (want, other) and sorted([want, other]) == sorted([[new[0], old[1], new[2]], [old[0], new[1], old[2]]])
    # the default chain: sets are joined, and the planted one keeps its sites and their arrangement
    assert 1 <= len(chain["joins"]) < chain["n_sets"]
    assert len({chain["ps2"][k] for k in h}) == 1 and letters(chain, chain["flip2"]) in (want, other)
    assert len({chain["flip"][k] ^ chain["flip2"][k] for k in h}) == 1
    # the texts are those of the parts
    assert chain["sets_tsv"].splitlines()[0] == ref.SETS_HEADER and len(chain["sets_tsv"].splitlines()) == 1 + chain["n_sets"]
    assert len(chain["joins_tsv"].splitlines()) == 1 + len(chain["joins"]) and len(chain["joined_tsv"].splitlines()) == 1 + len(chain["pos"])


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def sj_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sjisa") / "ph.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_phase.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel,lds", [("k_sj_bits", 0), ("k_sj_pairs", 2 * 32 * 32 * 8)])
def test_kernels_without_scratch(sj_isa, kernel, lds):
    """no scratch, no spill, and no LDS beyond the staged chunk of both ranges (32 bit rows of 32 sets, 8 bytes each, twice).  The
    fields of the code-object metadata only."""
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"\w*)\n", sj_isa):
        a = sj_isa.rfind("\n  - ", 0, m.start())
        b = sj_isa.find("\n  - ", m.end())
        entries.append(sj_isa[a:b if b >= 0 else len(sj_isa)])
    assert len(entries) == 1, (kernel, len(entries))
    for e in entries:
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", e).group(1))
        print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
        assert field("private_segment_fixed_size") == 0
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("wavefront_size") == 64 and field("group_segment_fixed_size") == lds
