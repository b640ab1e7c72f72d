"""CPU: the ring walks of the on-chip CG kernel keep their LDS gathers in flight IN THE EMITTED ISA.

A node slot's walk gathers p of the node's six neighbours from LDS and runs 26 fp64 FMAs on them.  At the register ceiling
of the four-slot kernels the scheduler had turned "all six gathers in one block" into gather, `s_waitcnt lgkmcnt(0)`, four
FMAs, six times per slot: six dependent LDS round trips with one other wave on the SIMD to cover them.  ring_walk_blocks
(cg_device.h) now issues the gathers in groups of G and pins each group in front of its FMAs; k_cg_persist derives G from
the instantiation (persist_kernel.h, persist_walk_group): two groups of three in the four-slot kernels on a grid, three
groups of two in the overflow one of the 512-node tiles, 0 -- the scheduler's placement, nothing pinned -- everywhere else: there the
scheduler keeps three to four gathers in flight by itself, and pinning all six up front measured slower.

Checked here, on the `make isa` listings, for every single-GPU edge-block instantiation of persist_shapes.h (all four
objects), in the walk region -- from the last `s_barrier` before the last `s_setprio 0` to that `s_setprio 0`, i.e. from the
barrier that ends the vector updates to the end of the last slot's walk:

  * every slot's walk (a basic block of the region with at least six `ds_read_b128`) has at least G gathers outstanding at
    the first `lgkmcnt` wait behind each group of gathers (G > 0);
  * no `scratch_load` in the region: a reload there waits for `vmcnt`, i.e. for the granule stores in flight;
  * `.vgpr_spill_count` is not above the count of the commit before the walks were pinned.

The listing is read for `ds_read_b128`, `s_waitcnt`, `scratch_load`, the labels and branches that delimit basic blocks, and
the kernels' metadata; nothing else."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "magnetite_amd", "csrc")
NB = 6  # kPersistBlockEntries: blocks per node in registers, gathers per walk

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="needs hipcc to emit the ISA")

# object -> (row list of persist_shapes.h, VAR, LC)
UNITS = {"persist": ("MAIN", 0, 0), "persist_k4": ("K4", 0, 0), "persist_cases": ("CASES", 0, 1),
         "persist_variants": ("CASES", 1, 1)}


def _rows(name):
    """The rows X(B, mg, ebm, one, nptx) of list MAG_PERSIST_ROWS_<name>."""
    text = open(os.path.join(CSRC, "persist_shapes.h")).read().replace("\\\n", " ")
    line = re.search(r"#define MAG_PERSIST_ROWS_%s\(X\)(.*)" % name, text).group(1)
    rows = re.findall(r"X\((\d+), (true|false), (\d), (true|false), (\d)\)", line)
    assert rows, name
    return [(int(b), mg == "true", int(ebm), one == "true", int(nptx)) for b, mg, ebm, one, nptx in rows]


def _cases():
    out = []
    for unit, (rows, var, lc) in UNITS.items():
        for b, mg, ebm, one, nptx in _rows(rows):
            if not mg and ebm >= 1:
                out.append((unit, b, ebm, one, nptx, var, lc))
    return out


CASES = _cases()


def expected_g(b, ebm, one, nptx):
    """persist_kernel.h, persist_walk_group, restated for one GPU: the four-slot kernels on a grid are pinned -- two groups of
    three, but three groups of two in the overflow kernel of the 512-node tiles; 0 = the scheduler's placement everywhere
    else (measured slower with all six pinned up front: DESIGN WG)."""
    if one or nptx != 0:
        return 0
    return 2 if ebm == 2 and b == 512 else 3


def parent_spills(unit, b, ebm, one, nptx):
    """.vgpr_spill_count of the commit before the walks were pinned: the four-slot structured kernel 5 (the structured kernel
    of the 256-node tiles 25), every other single-GPU edge-block instantiation 0."""
    if ebm == 1 and nptx == 0 and not one:
        return 5 if b == 512 else 25
    return 0


@pytest.fixture(scope="module")
def isa():
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "isa"], stdout=subprocess.DEVNULL)
    return {u: open(os.path.join(CSRC, "build", u + ".s")).read() for u in UNITS}


def _kernel(text, b, ebm, one, nptx, var, lc):
    name = "_ZN4magk12k_cg_persistILi%dELb0ELi512ELi%dELb%dELi%dELb%dELb%dEEEvNS_13PersistParamsE" % (b, ebm, one, nptx, var, lc)
    start = text.index("\n" + name + ":")
    body = text[start:text.index("\n.Lfunc_end", start)]
    meta = text[text.index(".name:           " + name + "\n"):]
    spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
    return [l.strip() for l in body.splitlines()], spills


def _region(lines):
    last = max(i for i, l in enumerate(lines) if l.startswith("s_setprio 0"))
    bar = max(i for i, l in enumerate(lines[:last]) if l.startswith("s_barrier"))
    return lines[bar:last + 1]


def _walks(region):
    """The basic blocks of the region with at least NB ds_read_b128, as lists of tokens: 'R' or the n of an lgkmcnt(n) wait."""
    blocks, cur = [], []
    for l in region:
        if re.match(r"\.LBB\d+_\d+:", l) or l.startswith(("s_cbranch", "s_branch")):
            blocks.append(cur)
            cur = []
        elif l.startswith("ds_read_b128"):
            cur.append("R")
        elif l.startswith("s_waitcnt"):
            m = re.search(r"lgkmcnt\((\d+)\)", l)
            if m:
                cur.append(int(m.group(1)))
    blocks.append(cur)
    return [b for b in blocks if b.count("R") >= NB]


def outstanding_at_group_waits(walk):
    """Gathers outstanding at the first wait behind each group of gathers (the counter starts at 0 with the block: p of the
    node itself, read before the branch into the walk, is not counted)."""
    out, c, fresh = [], 0, False
    for t in walk:
        if t == "R":
            c += 1
            fresh = True
        else:
            if fresh:
                out.append(c)
            c, fresh = min(c, t), False
    return out


def test_the_parser_on_the_patterns_this_is_about():
    serial = ["R", "R", 1, 0, "R", 0, "R", 0, "R", 0, "R", 0]  # the four-slot kernel before: one gather per round trip
    assert min(outstanding_at_group_waits(serial)) == 1
    assert outstanding_at_group_waits(["R", "R", "R", 2, 1, 0, "R", "R", "R", 2, 1, 0]) == [3, 3]
    assert outstanding_at_group_waits(["R", "R", "R", 1, "R", "R", "R", 3, 0]) == [3, 4]
    assert outstanding_at_group_waits(["R"] * 6 + [3, 0]) == [6]


@pytest.mark.parametrize("unit,b,ebm,one,nptx,var,lc", CASES, ids=["%s-%d-%d-%d-%d" % c[:5] for c in CASES])
def test_walks_keep_their_gathers_in_flight(isa, unit, b, ebm, one, nptx, var, lc):
    lines, spills = _kernel(isa[unit], b, ebm, one, nptx, var, lc)
    region = _region(lines)
    g = expected_g(b, ebm, one, nptx)
    walks = _walks(region)
    assert len(walks) == (nptx or 4), walks  # one walk per node slot (256-node tiles: four slots of 512 lanes as well)
    if g:  # (nothing to ask where the placement is the scheduler's)
        for k, wk in enumerate(walks):
            got = outstanding_at_group_waits(wk)
            assert got and min(got) >= g, (k, g, wk)
    assert not [l for l in region if l.startswith("scratch_load")]
    assert spills <= parent_spills(unit, b, ebm, one, nptx), spills
