"""--both-strands without a GPU: the ABI fields of vga_map_params.strands / vga_map_result.strand, the read simulator's
reverse reads, and the '-' GAF and validation records of the host writers."""
import ctypes as C
import hashlib
import os
import subprocess

from helpers import DATA, ROOT, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")


def test_strand_fields_of_the_abi(tmp_path):
    """strands sits in the tail padding of vga_map_params (size unchanged), strand is appended to vga_map_result; ctypes agrees
    and the default is forward"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vga_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d\\n", offsetof(vga_map_params, strands), sizeof(vga_map_params),\n'
                   '         offsetof(vga_map_result, strand), sizeof(vga_map_result), VGA_STRANDS_FORWARD, VGA_STRANDS_BOTH);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [28, 32, 144, 152, 0, 1]
    b = pkg().binding
    assert b.MapParams.strands.offset == 28 and C.sizeof(b.MapParams) == 32
    assert b.MapResult.strand.offset == 144 and C.sizeof(b.MapResult) == 152
    assert (b.VGA_STRANDS_FORWARD, b.VGA_STRANDS_BOTH) == (0, 1)
    p = b.MapParams()
    p.strands = 5
    b.load_library().vga_map_default_params(C.byref(p))
    assert p.strands == 0


def _digest(reads):
    return hashlib.sha256("".join(f">{r.name}\t{r.path}\t{r.offset}\t{r.template_len}\n{r.seq}\n" for r in reads).encode()).hexdigest()


def test_readsim_reverse_reads():
    rs = pkg().readsim
    # the first 50 reads of config 3 as the simulator drew them before it had reverse reads
    want = "ac32f1fcda86f79bc2643bb9efc32accaf1d7c98c6c10110f0587c43c5c29e23"
    fwd = rs.simulate_reads(DRB1, 50, 10000, 0.03, 0.03, 0.04, seed=77, reverse_fraction=0.0)
    assert _digest(rs.config3_reads(DRB1, 50)) == _digest(fwd) == want
    assert all(r.strand == "+" for r in fwd)
    mixed = rs.simulate_reads(DRB1, 50, 10000, 0.03, 0.03, 0.04, seed=77, reverse_fraction=0.5)
    assert _digest(mixed) == _digest(rs.simulate_reads(DRB1, 50, 10000, 0.03, 0.03, 0.04, seed=77, reverse_fraction=0.5))
    n_minus = 0
    for m, f in zip(mixed, fwd):
        assert (m.name, m.path, m.offset, m.template_len) == (f.name, f.path, f.offset, f.template_len)
        if m.strand == "-":
            n_minus += 1
            assert m.seq == rs.reverse_complement(f.seq) and rs.reverse_complement(m.seq) == f.seq
        else:
            assert m.strand == "+" and m.seq == f.seq
    assert 10 < n_minus < 40
    tm, tf = rs.truth_gaf(DRB1, mixed).splitlines(), rs.truth_gaf(DRB1, fwd).splitlines()
    for m, a, b in zip(mixed, tm, tf):
        x, y = a.split("\t"), b.split("\t")
        assert x[4] == m.strand and x[:4] + x[5:] == y[:4] + y[5:]
    # switch_base (src/dna.rs:20-33): U / u pair with A / a, any other byte becomes N
    assert rs.reverse_complement("ACGTUacgtuNx-") == "NNNaacgtAACGT"


def test_reverse_strand_gaf_records():
    """rule 5: a '-' chain record has qs = L - (query_begin[last] + k), qe = L - query_begin[first]; a '-' alignment record
    differs from the '+' one in column 5 only"""
    hl = pkg().hostlib
    path = "(>3:4,>3:14),(>5:0,>5:10),"
    plus = hl.gaf_chain_record("r1", 1000, 11, 0, [100, 250, 300], path).rstrip("\n").split("\t")
    minus = hl.gaf_chain_record("r1", 1000, 11, 1, [100, 250, 300], path).rstrip("\n").split("\t")
    assert plus[:6] == ["r1", "1000", "100", "311", "+", path]
    assert minus[:6] == ["r1", "1000", "689", "900", "-", path]
    assert minus[6:] == plus[6:] == ["0", "0", "0", "0", "0", "0", "ta:Z:chain,n_anchors: 3"]
    args = ([2 << 1, 3 << 1, 5 << 1], 40, 3, 30, 27, "cs:Z::27", "27M")
    a_plus = hl.gaf_alignment_record_strand("r1", 27, False, *args).split("\t")
    a_minus = hl.gaf_alignment_record_strand("r1", 27, True, *args).split("\t")
    assert a_plus == hl.gaf_alignment_record("r1", 27, True, *args).split("\t")
    assert a_plus[2:6] == ["0", "27", "+", ">2>3>5"] and a_minus[4] == "-"
    assert a_minus[:4] + a_minus[5:] == a_plus[:4] + a_plus[5:]


def test_reverse_strand_validation_record():
    """rule 6: the validation record of a '-' alignment carries the reverse complement of the read"""
    p = pkg()
    hi = p.HostIndex.build_from_gfa(DRB1, 11)
    seq = "ACGTTGCAAG"
    rec = "\t".join(["r1", "10", "0", "10", "%s", ">1", "10", "0", "10", "0", "10", "255", "as:i:-30 cs:Z::10,cg:Z:10M"])
    plus = hi.validation_records(rec % "+" + "\n", ["r1"], [seq])
    minus = hi.validation_records(rec % "-" + "\n", ["r1"], [seq])
    assert plus.split("\n")[2] == seq
    assert minus.split("\n")[2] == p.readsim.reverse_complement(seq) == "CTTGCAACGT"
    assert minus.split("\n")[:2] + minus.split("\n")[3:] == plus.split("\n")[:2] + plus.split("\n")[3:]
