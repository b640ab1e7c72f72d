"""CPU: the update phase of the on-chip CG kernel keeps its LDS loads in flight IN THE EMITTED ISA.

An iteration of k_cg_persist (persist_kernel.h) opens with the scalars -- alpha, beta, the cost: two divisions and a square root,
some forty dependent fp64 operations in every wave -- and the vector updates of the lane's four node slots: r += alpha q,
p = beta p - r, with p and q of the slot read from LDS.  At the register ceiling of the four-slot kernels the scheduler had
emitted the updates as load, load, `s_waitcnt lgkmcnt(0)`, four FMAs, store, once per slot, behind the scalars: four dependent
LDS round trips that wait for nothing they need.  Where persist_update_loads says so (DESIGN UB) q of the four slots is read
at the top of the loop body, in front of the scalars, and p two slots at a time in front of the r updates of two slots, with
counted waits.

Checked here, on the `make isa` listings, for every single-GPU edge-block instantiation of persist_shapes.h (all four
objects), in the update region -- the CG loop from its header to the `s_barrier` that ends the updates, the barrier
tests/test_walk_gathers_isa.py's region starts at -- along the path of a steady-state iteration of a wave whose slots are all
live (`follow`, below):

  * where the new shape is on: four `ds_read_b128` are issued in front of the first `v_rcp_f64`; behind the scalars, at the
    first `lgkmcnt` wait behind each group of reads of the own-slot updates at least four reads are outstanding; no
    `scratch_` instruction in the region; `.vgpr_spill_count` <= 4, `.vgpr_count` <= 256, `.sgpr_spill_count` <= 69;
  * everywhere else: the region's tokens are the parent commit's, token for token (tests/golden/update_loads_parent_tokens.json).

The listing is read for `ds_read_b128`, `ds_write_b128`, `s_waitcnt`, `v_rcp_f64`, `v_rsq_f64`, `s_barrier`, `scratch_*`, labels,
branches and the kernels' metadata; nothing else."""
import heapq
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "magnetite_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "update_loads_parent_tokens.json")
NPT = 4  # node slots per lane of the kernels the new shape is for

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
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


def expected_front(b, ebm, one, nptx):
    """persist_kernel.h, persist_update_loads, restated for one GPU: the `ds_read_b128` in front of the scalars -- q of the four
    node slots -- in the four-slot structured kernel of the 512-node tiles on a grid; None: the shape is off."""
    if one or nptx != 0 or b != 512 or ebm != 1:
        return None
    return 4


def case_id(c):
    return "%s-%d-%d-%d-%d" % c[:5]


@pytest.fixture(scope="module")
def isa():
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "isa"], stdout=subprocess.DEVNULL)
    return {u: open(os.path.join(CSRC, "build", u + ".s")).read() for u in UNITS}


def _kernel(text, b, ebm, one, nptx, var, lc):
    name = "_ZN4magk12k_cg_persistILi%dELb0ELi512ELi%dELb%dELi%dELb%dELb%dEEEvNS_13PersistParamsE" % (b, ebm, one, nptx, var, lc)
    start = text.index("\n" + name + ":")
    body = text[start:text.index("\n.Lfunc_end", start)]
    meta = text[text.index(".name:           " + name + "\n"):]
    counts = {k: int(re.search(r"\.%s:\s+(\d+)" % k, meta).group(1)) for k in ("vgpr_spill_count", "vgpr_count", "sgpr_spill_count")}
    return [l.strip() for l in body.splitlines()], counts


def _label(l):
    m = re.match(r"(\.LBB\d+_\d+):", l)
    return m.group(1) if m else None


def _bounds(lines):
    """(loop header, the barrier that ends the updates): the barrier as test_walk_gathers_isa._region finds it, the header the
    last loop header of depth 1 in front of it whose loop the barrier lies in -- the CG loop."""
    last = max(i for i, l in enumerate(lines) if l.startswith("s_setprio 0"))
    bar = max(i for i, l in enumerate(lines[:last]) if l.startswith("s_barrier"))
    head = max(i for i, l in enumerate(lines[:bar]) if _label(l) and "Loop Header: Depth=1" in l)
    return head, bar


def _token(l):
    if l.startswith("ds_read_b128"):
        return "R"
    if l.startswith("ds_write_b128"):
        return "W"
    if l.startswith("v_rcp_f64"):
        return "rcp"
    if l.startswith("v_rsq_f64"):
        return "rsq"
    if l.startswith("scratch_"):
        return "S"
    if l.startswith("s_waitcnt"):
        m = re.search(r"lgkmcnt\((\d+)\)", l)
        if m:
            return int(m.group(1))
    return None


def _block_has_b128(lines, i):
    """Does the basic block that starts at line i hold a 16-byte LDS access?"""
    for l in lines[i:]:
        if l.startswith(("ds_read_b128", "ds_write_b128")):
            return True
        if _label(l) or l.startswith(("s_cbranch", "s_branch", "s_barrier")):
            return False
    return False


def follow(lines, head, bar):
    """The tokens along the path of a steady-state iteration from line `head` to the barrier at line `bar`:

      * a branch on EXEC (`s_cbranch_execz`, `s_cbranch_execnz`) guards a block of lanes: the path enters the block when it holds a
        16-byte LDS access -- a node slot's or a halo entry's update, which the wave followed has lanes for -- and jumps over
        it otherwise (the blocks of the one reporting lane: cost history, best cost);
      * at a scalar branch (`s_cbranch_scc*`, `s_cbranch_vcc*`) the path takes the SHORTER way to the barrier, in instructions:
        the first iteration's block, the verdicts' exits, and x += alpha p on the critical path (beta == 0) are all jumped over;
        so is, where there are two, the update with a test per slot in favour of the all-live one.
    """
    labels = {_label(l): i for i, l in enumerate(lines) if _label(l)}

    def succ(i):
        l = lines[i]
        if i == bar or l.startswith("s_endpgm"):
            return []
        if l.startswith("s_branch"):
            return [labels[l.split()[1]]]
        if l.startswith(("s_cbranch_execz", "s_cbranch_execnz")):
            t = labels[l.split()[1]]
            inside, around = (i + 1, t) if l.startswith("s_cbranch_execz") else (t, i + 1)
            return [inside if _block_has_b128(lines, inside + (1 if _label(lines[inside]) else 0)) else around]
        if l.startswith("s_cbranch"):
            return [i + 1, labels[l.split()[1]]]
        return [i + 1] if i + 1 < len(lines) else []

    dist, prev, heap = {head: 0}, {}, [(0, head)]
    while heap:
        d, i = heapq.heappop(heap)
        if i == bar:
            break
        if d > dist[i]:
            continue
        for j in succ(i):
            if j not in dist or d + 1 < dist[j]:
                dist[j], prev[j] = d + 1, i
                heapq.heappush(heap, (d + 1, j))
    assert bar in dist, "no path from the loop header to the barrier"
    path, i = [bar], bar
    while i != head:
        i = prev[i]
        path.append(i)
    return [t for t in (_token(lines[i]) for i in reversed(path)) if t is not None]


def reads_in_front(tokens):
    """`ds_read_b128` issued in front of the first `v_rcp_f64`."""
    return tokens[:tokens.index("rcp")].count("R")


def own_slot_tokens(tokens, slots=NPT):
    """The own-slot updates: behind the scalars (the last `v_rcp_f64` / `v_rsq_f64`) up to the store of the last slot -- a
    slot's update ends with ONE `ds_write_b128` (p), a halo entry's with two (r and p) --, with the reads that were in flight
    when the scalars began in front."""
    end = max(i for i, t in enumerate(tokens) if t in ("rcp", "rsq"))
    first = tokens.index("rcp")
    early = ["R"] * tokens[:first].count("R")
    rest, out, w = tokens[end + 1:], [], 0
    for t in rest:
        out.append(t)
        if t == "W":
            w += 1
            if w == slots:
                break
    assert w == slots, tokens
    return early + out


def outstanding_at_group_waits(tokens):
    """Reads outstanding at the first `lgkmcnt` wait behind each group of reads (tests/test_walk_gathers_isa.py's count: a wait
    for n leaves at most n outstanding)."""
    out, c, fresh = [], 0, False
    for t in tokens:
        if t == "R":
            c += 1
            fresh = True
        elif isinstance(t, int):
            if fresh:
                out.append(c)
            c, fresh = min(c, t), False
    return out


def test_the_parser_on_the_patterns_this_is_about():
    parent = ["rsq", "rcp", "rcp"] + ["R", "R", 0, "W"] * 4 + ["R", "R", 1, 0, "W", "W"]
    assert reads_in_front(parent) == 0
    assert own_slot_tokens(parent) == ["R", "R", 0, "W"] * 4
    assert outstanding_at_group_waits(["R", "R", 0, "W", "R", "R", 0, "W", "R", "R", 0, "W", "R", "R", 0, "W"]) == [2, 2, 2, 2]
    together = ["R"] * 8 + ["rcp", "rcp", "rsq", 6, "W", 5, "W", 4, 2, "W", "W", "R", "R", 1, 0, "W", "W"]
    assert reads_in_front(together) == 8 and outstanding_at_group_waits(own_slot_tokens(together)) == [8]
    two_groups = ["R"] * 4 + ["rcp", "rcp", "rsq", "R", "R", 4, "W", 2, "W", "R", "R", 2, "W", 0, "W", "R", "R", 1, 0, "W", "W"]
    assert reads_in_front(two_groups) == 4 and outstanding_at_group_waits(own_slot_tokens(two_groups)) == [6, 4]
    # this commit's: q of four slots in front, p in pairs
    q_first = ["R"] * 4 + ["rcp", "rcp", "rsq", "R", "R", 5, 4, "R", "R", 5, 3, "W", 3, "W", 3, "W", 3, "W", "R", "R", 1, 0, "W", "W"]
    assert reads_in_front(q_first) == 4 and outstanding_at_group_waits(own_slot_tokens(q_first)) == [6, 6]
    # a load that has to wait for its destination registers -- the sources of a store still in flight -- breaks a group up
    reused = ["R"] * 4 + ["rcp", "rcp", "rsq", "R", "R", 4, "W", 2, "W", 3, "R", 3, "R", 2, "W", 0, "W"]
    assert min(outstanding_at_group_waits(own_slot_tokens(reused))) == 3
    # the path: into the lanes' blocks that hold 16-byte LDS accesses, round the reporter's, the shorter way at scalar branches
    lines = [".LBB0_1: ; =>This Loop Header: Depth=1", "ds_read_b128 v[0:3], v9", "v_rcp_f64_e32 v[4:5], v[6:7]",
             "s_cbranch_execz .LBB0_3", "ds_read_b64 v[4:5], v9", "s_waitcnt lgkmcnt(0)", ".LBB0_3:", "s_cbranch_scc1 .LBB0_5",
             "ds_read_b128 v[0:3], v9", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v0, 0", "ds_write_b128 v9, v[0:3]", ".LBB0_5:",
             "s_cbranch_execnz .LBB0_8", ".LBB0_6:", "s_waitcnt lgkmcnt(0)", "s_barrier", ".LBB0_8:", "s_waitcnt lgkmcnt(0)",
             "ds_write_b128 v9, v[0:3]", "s_branch .LBB0_6"]
    assert follow(lines, 0, 16) == ["R", "rcp", 0, "W", 0]


@needs_hipcc
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_update_loads_are_in_flight_under_the_scalars(isa, case):
    unit, b, ebm, one, nptx, var, lc = case
    lines, counts = _kernel(isa[unit], b, ebm, one, nptx, var, lc)
    head, bar = _bounds(lines)
    tokens = follow(lines, head, bar)
    front = expected_front(b, ebm, one, nptx)
    if front is None:  # the shape is off: the parent's region, token for token
        golden = json.load(open(GOLDEN))
        assert " ".join(str(t) for t in tokens) == golden[case_id(case)], tokens
        return
    assert front >= 4 and reads_in_front(tokens) == front, tokens
    got = outstanding_at_group_waits(own_slot_tokens(tokens))
    assert got and min(got) >= 4, (got, tokens)
    assert not [l for l in lines[head:bar + 1] if l.startswith("scratch_")]
    assert "S" not in tokens
    assert counts["vgpr_spill_count"] <= 4 and counts["vgpr_count"] <= 256, counts
    assert counts["sgpr_spill_count"] <= 69, counts  # the parent's: SGPR reloads are v_readlane in the loop
