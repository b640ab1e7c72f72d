"""CPU: the CG loop of the four-slot structured on-chip kernel keeps its bookkeeping out of the vector pipe IN THE EMITTED ISA
(persist_kernel.h, persist_loop_scalars; DESIGN LS).

With 512-node tiles and 512 threads a node slot IS a tile and a lane's position in it IS its thread index.  The loop computed
both from `s * THREADS + tid` all the same -- a v_readfirstlane_b32 of that register, a signed division, an s_mul_i32 by the
tile's words in front of every LDS access -- and kept the loop-invariant lane masks of the node flags in 61 spilled SGPRs that
came back through v_readlane_b32 in front of every use.  Now tile and position are compile-time, and what a wave needs to know of
its slots' flags are bits of one scalar word.

Checked on the `make isa` listing of persist_k4 (the one kernel the predicate is on for), in the CG loop -- the header that
tests/test_exchange_reduction_isa.py's cut finds to the back edge, both arms of every branch counted:

  * no `v_readfirstlane_b32` whose source is a thread-index register: the register the prologue makes by `v_and_b32 .., 0x3ff, v0`,
    or one it makes from that by adding a constant (the parent's `s * THREADS + tid`);
  * `.vgpr_spill_count` is 0 and the loop holds no `scratch_` instruction;
  * the loop's `v_readlane_b32` + `v_readfirstlane_b32`, its `s_mul_i32`, all its vector instructions, and the kernel's
    `.sgpr_spill_count` are each strictly below the parent commit's (tests/golden/loop_scalars_parent_counts.json, counted by
    this file's walker on the parent commit's listing).

The listing is read for mnemonics, labels, branches and the kernel's metadata; nothing else."""
import json
import os
import re
import shutil
import subprocess

import pytest

import test_exchange_batched_isa as xb
import test_exchange_reduction_isa as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "magnetite_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "loop_scalars_parent_counts.json")
K4 = "_ZN4magk12k_cg_persistILi512ELb0ELi512ELi1ELb0ELi0ELb0ELb0EEEvNS_13PersistParamsE"

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="needs hipcc to emit the ISA")


@pytest.fixture(scope="module")
def listing():
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "isa"], stdout=subprocess.DEVNULL)
    return open(os.path.join(CSRC, "build", "persist_k4.s")).read()


def loop_of(lines):
    """(first, last) line numbers of the CG loop: its header to the branch back to it."""
    head, _, _, _, back = xr.cut(lines)
    return head, back


def _mnemonic(l):
    return l.split()[0] if l and not l.startswith((";", ".")) and not xb._label(l) else None


def _regs(l):
    """Operands of an instruction line: ['v1', 's[2:3]', '0x3ff', ...]."""
    return [o.strip() for o in l.split(None, 1)[1].split(",")] if len(l.split(None, 1)) > 1 else []


def thread_index_registers_at(lines, i):
    """The VGPRs that hold the thread index, or the thread index plus a constant, at line i: followed from the kernel's first
    line along the text -- `v_and_b32 vX, 0x3ff, v0` makes one, `v_add_u32 / v_or_b32 vY, <constant>, vX` makes another from
    one, any other write of a register takes it out."""
    held = set()
    for l in lines[:i]:
        m = _mnemonic(l)
        if not m or not m.startswith(("v_", "ds_read", "global_load", "buffer_load", "scratch_load")):
            continue
        ops = _regs(l)
        if not ops or not re.fullmatch(r"v\d+", ops[0]):
            if ops:  # a register tuple written: its members no longer hold the index
                t = re.fullmatch(r"v\[(\d+):(\d+)\]", ops[0])
                if t:
                    held -= {"v%d" % k for k in range(int(t.group(1)), int(t.group(2)) + 1)}
            continue
        dst = ops[0]
        if m.startswith("v_and_b32") and ops[1:] == ["0x3ff", "v0"]:
            held.add(dst)
        elif m.startswith(("v_add_u32", "v_or_b32")) and len(ops) == 3 and re.fullmatch(r"(0x[0-9a-f]+|\d+)", ops[1]) and ops[2] in held:
            held.add(dst)
        elif m.startswith("v_mov_b32") and len(ops) == 2 and ops[1] in held:
            held.add(dst)
        elif not m.startswith(("v_cmp", "v_readlane", "v_readfirstlane")):  # (those write no VGPR)
            held.discard(dst)
    return held


def readfirstlanes_of_the_thread_index(lines):
    first, last = loop_of(lines)
    return [l for i, l in enumerate(lines[first:last + 1], first)
            if l.startswith("v_readfirstlane_b32") and _regs(l)[1] in thread_index_registers_at(lines, i)]


def counts(lines):
    first, last = loop_of(lines)
    body = [m for m in map(_mnemonic, lines[first:last + 1]) if m]
    return {"lane_reads": sum(m in ("v_readlane_b32", "v_readfirstlane_b32") for m in body),
            "s_mul_i32": body.count("s_mul_i32"),
            "vector_instructions": sum(m.startswith("v_") for m in body)}


def metadata(text, key):
    meta = text[text.index(".name:           " + K4 + "\n"):]
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def test_the_walker_on_the_patterns_this_is_about():
    r, w = "buffer_load_dwordx4 v[4:7], v8, s[4:7], 0 offen sc1", "s_waitcnt vmcnt(%d)"
    prologue = ["v_and_b32_e32 v74, 0x3ff, v0", "v_add_u32_e32 v227, 0x200, v74", "v_or_b32_e32 v6, 0x400, v74",
                "v_add_u32_e32 v33, 0x600, v74", "v_mov_b32_e32 v9, v74", "v_lshlrev_b32_e32 v9, 4, v9"]
    head = [".LBB0_1:                                ; =>This Loop Header: Depth=1", "%s",
            "s_barrier", ".LBB0_2:                         ;   in Loop: Header=BB0_1 Depth=1", "s_sleep 8", "s_sleep 6"]
    poll = [".LBB0_3:                                ;   Parent Loop BB0_1 Depth=1", r, r, w % 1, w % 0,
            "s_cbranch_scc1 .LBB0_4", "s_sleep 1", "s_branch .LBB0_3", ".LBB0_4:                         ;   in Loop: Header=BB0_1 Depth=1"]
    tail = [w % 0, "ds_write_b64 v1, v[2:3]", "s_barrier", "ds_read_b128 v[4:7], v1", "v_readlane_b32 s4, v2, 15",
            "s_cbranch_vccz .LBB0_9", "s_branch .LBB0_1", ".LBB0_9:", "v_readfirstlane_b32 s5, v74", "s_mul_i32 s5, s5, s6", "s_endpgm"]

    def kernel(first):
        return prologue + [l % first if "%s" in l else l for l in head] + poll + tail

    # the parent: the tile of slot 1 from the thread index, a division, a multiplication by the tile's words
    parent = [x for l in kernel("%s") for x in (["v_readfirstlane_b32 s5, v227", "s_ashr_i32 s6, s5, 31", "s_mul_i32 s5, s5, s7",
                                                 "v_mov_b32_e32 v3, s5"] if l == "%s" else [l])]
    assert readfirstlanes_of_the_thread_index(parent) == ["v_readfirstlane_b32 s5, v227"]
    assert counts(parent) == {"lane_reads": 2, "s_mul_i32": 1, "vector_instructions": 3}  # (what stands behind the loop is not counted)
    # this change: no such read; a readfirstlane of a value computed in the loop is none of the thread index
    own = [x for l in kernel("%s") for x in (["v_add_f64 v[2:3], v[2:3], v[4:5]", "v_readfirstlane_b32 s5, v3"] if l == "%s" else [l])]
    assert readfirstlanes_of_the_thread_index(own) == []
    assert counts(own) == {"lane_reads": 2, "s_mul_i32": 0, "vector_instructions": 3}
    # a copy of the thread index is the thread index; a register written anew is not
    copy = [x for l in kernel("%s") for x in (["v_readfirstlane_b32 s5, v9"] if l == "%s" else [l])]
    assert readfirstlanes_of_the_thread_index(copy) == []  # v9 was shifted in the prologue
    copy = [x for l in kernel("%s") for x in (["v_mov_b32_e32 v9, v6", "v_readfirstlane_b32 s5, v9"] if l == "%s" else [l])]
    assert readfirstlanes_of_the_thread_index(copy) == ["v_readfirstlane_b32 s5, v9"]
    # a tuple load over a held register takes it out
    over = [x for l in kernel("%s") for x in (["ds_read_b128 v[4:7], v1", "v_readfirstlane_b32 s5, v6"] if l == "%s" else [l])]
    assert readfirstlanes_of_the_thread_index(over) == []


def test_no_lane_read_of_the_thread_index_and_no_scratch_in_the_loop(listing):
    lines, spills = xb._kernel(listing, 512, 1, 0, 0, 0)
    assert readfirstlanes_of_the_thread_index(lines) == []
    assert spills == 0 and metadata(listing, "vgpr_spill_count") == 0
    assert xr.loop_scratch(lines) == []


def test_the_loop_issues_less_than_the_parents(listing):
    parent = json.load(open(GOLDEN))
    lines, _ = xb._kernel(listing, 512, 1, 0, 0, 0)
    got = dict(counts(lines), sgpr_spill_count=metadata(listing, "sgpr_spill_count"))
    print(got, parent)
    for key in ("lane_reads", "s_mul_i32", "vector_instructions", "sgpr_spill_count"):
        assert got[key] < parent[key], (key, got[key], parent[key])
