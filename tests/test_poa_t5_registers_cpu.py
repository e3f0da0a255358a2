"""Register budget of k_poa_dp_t5<256, true>, from a cross-compile of vga_poa.hip for gfx950 with -DPOA_MARKERS.

The kernel runs at five waves per SIMD (at most 96 VGPRs); scalars that do not fit the scalar register file are spilled into
VGPR lanes and every reload is a v_readlane, one VALU slot of an issue-bound kernel.  These checks keep a later edit from
quietly bringing those reloads back onto the rows' common path:
  * the SGPR spill count stays under a ceiling (181 before the row loop's state was narrowed);
  * the scratch size stays under a ceiling (12 B before);
  * spill-lane moves (v_readlane / v_writelane on a spill VGPR) in the row loop's common regions stay under a ceiling;
  * the hot step loop (the interior of a simple row) has no spill-lane move at all.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "k_poa_dp_t5ILi256ELb1"
SGPR_SPILL_CEILING = 135
SCRATCH_CEILING = 8
COMMON_MOVES_CEILING = 100
COMMON = ("row_topo", "row_prevmax", "row_setup", "row_steps", "row_end")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
    out = str(tmp_path_factory.mktemp("t5isa") / "vga_poa_marked.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-DPOA_MARKERS", "-S",
                           "--cuda-device-only", "-I", csrc, os.path.join(csrc, "vga_poa.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"_Z\d+" + KERNEL + r".*:", l))
    name = lines[start].split(":")[0]
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    k = text.index(".amdhsa_kernel " + name)
    desc = text[k:text.index(".end_amdhsa_kernel", k)]
    # the metadata entry of this kernel: the block whose .name is the mangled name
    m = re.search(r"\.name:\s+" + re.escape(name) + r"\n", text)
    entry_start = text.rfind("\n  - ", 0, m.start())
    entry_end = text.find("\n  - ", m.end())
    entry = text[entry_start:entry_end if entry_end >= 0 else len(text)]
    return dict(lines=lines[start:end], desc=desc, entry=entry)


def _spill_vgprs(lines):
    return set(re.findall(r"v_writelane_b32 (v\d+),", "\n".join(lines)))


def _is_spill_move(t, spill):
    m = re.match(r"v_(?:readlane|writelane)_b32 (\w+), (\w+)", t)
    return bool(m) and (m.group(1) in spill or m.group(2) in spill)


def _moves_by_region(lines):
    spill = _spill_vgprs(lines)
    region, cnt = "prologue", collections.Counter()
    for l in lines:
        t = l.strip()
        m = re.match(r"; MARK (\w+)", t)
        if m:
            region = m.group(1)
            continue
        if t and not t.startswith((";", ".")) and not t.endswith(":") and _is_spill_move(t, spill):
            cnt[region] += 1
    return cnt


def _loops(lines):
    """Instructions per innermost loop (header label -> (depth, markers seen, instruction lines)), from the loop comments."""
    loops = collections.defaultdict(lambda: [0, set(), []])
    cur = None
    for i, l in enumerate(lines):
        t = l.strip()
        h = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", l)
        m = re.search(r"in Loop: Header=BB(\d+_\d+) Depth=(\d+)", l)
        if h:
            j = i
            while not lines[j].strip().startswith(".LBB"):
                j -= 1
            cur = re.match(r"\.LBB(\d+_\d+)", lines[j].strip()).group(1)
            loops[cur][0] = int(h.group(1))
            continue
        if m:
            cur = m.group(1)
            loops[cur][0] = int(m.group(2))
            continue
        if t.startswith(".LBB") or t.startswith("; %bb."):
            cur = None  # a block outside every loop (a loop block carries an "in Loop" comment on its label line)
            continue
        mk = re.match(r"; MARK (\w+)", t)
        if mk:
            if cur is not None:
                loops[cur][1].add(mk.group(1))
            continue
        if cur is not None and t and not t.startswith((";", ".")):
            loops[cur][2].append(t)
    return loops


def test_no_scratch_growth(isa):
    size = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", isa["desc"]).group(1))
    assert size <= SCRATCH_CEILING, size


def test_sgpr_spills_under_ceiling(isa):
    spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", isa["entry"]).group(1))
    assert spills <= SGPR_SPILL_CEILING, spills


def test_common_row_regions_keep_few_spill_moves(isa):
    cnt = _moves_by_region(isa["lines"])
    assert "row_setup" in cnt or "row_topo" in cnt or sum(cnt.values()) > 0  # the markers are there
    common = sum(v for r, v in cnt.items() if r in COMMON or r.startswith("hot_"))
    assert common <= COMMON_MOVES_CEILING, dict(cnt)


def test_hot_step_loop_has_no_spill_moves(isa):
    spill = _spill_vgprs(isa["lines"])
    loops = _loops(isa["lines"])
    hot = [h for h, (depth, marks, _) in loops.items() if "hot_p2_fast" in marks and "row_topo" not in marks and depth >= 2]
    # the innermost loop that holds the hot phase 2: the step loop of hot rows
    hot = [h for h in hot if loops[h][0] == max(loops[x][0] for x in hot)]
    assert len(hot) == 1, {h: (loops[h][0], sorted(loops[h][1])) for h in hot}
    moves = [t for t in loops[hot[0]][2] if _is_spill_move(t, spill)]
    assert not moves, moves
