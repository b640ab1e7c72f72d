"""CPU: the exchange of the four-slot structured on-chip CG kernel reduces the records on each lane's own piece and meets at ONE
workgroup barrier IN THE EMITTED ISA (persist_kernel.h, persist_exchange<.., XR>; persist_own_piece_reduction; DESIGN XR).

Lane `tid` of the 512-thread exchange validates record piece `tid`, and the reduction tree read exactly that piece back for it
from LDS behind a barrier of its own.  Now the piece stays in registers, a wave runs the first half of the tree when its own
sweep has ended, and flags and partials cross the workgroup at one barrier.

Checked on the `make isa` listing of persist_k4 (the one kernel the predicate is on for), in the CG loop's exchange, cut out
as tests/test_exchange_batched_isa.py cuts it -- the last pair of `s_sleep` of the kernel and the barriers around it:

  * exactly one `s_barrier` between the sweep's last `s_waitcnt vmcnt` and the CG loop's back edge;
  * no `ds_write` inside the polling loop (the sleeps to the sweep's last backward branch);
  * `.vgpr_spill_count` is at most the parent commit's 3, and the CG loop holds no scratch instruction the parent's does not
    have (the parent's: three dword reloads at offsets 0, 4, 8);
  * persist, persist_cases and persist_variants, where the predicate is off: every kernel's `.vgpr_count` and
    `.vgpr_spill_count` are the parent commit's (tests/golden/exchange_reduction_parent_registers.json).

The listing is read for those mnemonics, labels, branches and the kernels' metadata; nothing else."""
import json
import os
import re
import shutil
import subprocess

import pytest

import test_exchange_batched_isa as xb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "magnetite_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "exchange_reduction_parent_registers.json")
PARENT_SPILLS = 3
PARENT_LOOP_SCRATCH = {("scratch_load_dword", 0), ("scratch_load_dword", 4), ("scratch_load_dword", 8)}
OTHER_UNITS = ("persist", "persist_cases", "persist_variants")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="needs hipcc to emit the ISA")


@pytest.fixture(scope="module")
def isa():
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "isa"], stdout=subprocess.DEVNULL)
    return {u: open(os.path.join(CSRC, "build", u + ".s")).read() for u in OTHER_UNITS + ("persist_k4",)}


def _target(l):
    return l.split()[1] if l.startswith(("s_branch", "s_cbranch")) else None


def cut(lines):
    """Line numbers of the loop's exchange: (CG loop header, the sleeps, the sweep's last backward branch, the sweep's last
    vmcnt wait, the CG loop's back edge).  The header is the label the block of the sleeps names as its loop's."""
    _, pair, end = xb._bounds(lines)
    labels = {xb._label(l): i for i, l in enumerate(lines) if xb._label(l)}
    m = next(m for m in (re.search(r"in Loop: Header=(BB\d+_\d+) Depth=1", l) for l in reversed(lines[:pair])) if m)
    header = ".L" + m.group(1)
    back = min(i for i in range(end, len(lines)) if _target(lines[i]) == header)
    poll_end = max(i for i in range(pair, back) if _target(lines[i]) in labels and pair < labels[_target(lines[i])] < i)
    last_wait = max(i for i in range(pair, end) if xb._is_vmwait(lines[i]))
    assert poll_end < last_wait or not any(xb._is_load(l) for l in lines[last_wait:back]), "a granule load behind the last wait"
    return labels[header], pair, poll_end, last_wait, back


def barriers_behind_the_sweep(lines):
    _, _, _, last_wait, back = cut(lines)
    return sum(l.startswith("s_barrier") for l in lines[last_wait:back])


def lds_writes_in_the_polling_loop(lines):
    _, pair, poll_end, _, _ = cut(lines)
    return [l for l in lines[pair:poll_end + 1] if l.startswith("ds_write")]


def loop_scratch(lines):
    """(mnemonic, offset) of every scratch instruction of the CG loop: the header to the last branch back to it, and the blocks
    laid out behind it that say they are the loop's."""
    head, _, _, _, back = cut(lines)
    name = xb._label(lines[head])
    last = max(i for i in range(back, len(lines)) if _target(lines[i]) == name)
    body = lines[head:last + 1]
    inside = False
    for l in lines[last + 1:]:
        if xb._label(l):
            inside = ("Header=" + name[2:] + " ") in l
        elif inside:
            body.append(l)
    out = []
    for l in body:
        if l.startswith("scratch_"):
            m = re.search(r"offset:(\d+)", l)
            out.append((l.split()[0], int(m.group(1)) if m else 0))
    return out


def test_the_walker_on_the_patterns_this_is_about():
    r, w = "buffer_load_dwordx4 v[4:7], v8, s[4:7], 0 offen sc1", "s_waitcnt vmcnt(%d)"
    head = [".LBB0_1:                                ; =>This Loop Header: Depth=1", "v_fma_f64 v[0:1], v[2:3], v[4:5], v[0:1]",
            "s_barrier", ".LBB0_2:                         ;   in Loop: Header=BB0_1 Depth=1", "s_sleep 8", "s_sleep 6"]
    poll = [".LBB0_3:                                ;   Parent Loop BB0_1 Depth=1", r, r, w % 1, w % 0, "%s",
            "s_cbranch_scc1 .LBB0_4", "s_sleep 1", "s_branch .LBB0_3", ".LBB0_4:                         ;   in Loop: Header=BB0_1 Depth=1"]
    store = "ds_write_b128 v9, v[4:7]"
    # the parent: the piece to LDS in the loop, the flag barrier, half a tree, the partials' barrier
    parent = head + [l % store if "%s" in l else l for l in poll] + \
        [w % 0, "ds_write_b32 v1, v2", "s_barrier", "ds_read_b128 v[4:7], v9", "ds_write_b64 v1, v[2:3]", "s_barrier",
         "ds_read_b128 v[4:7], v1", "scratch_load_dword v13, off, off offset:4", "s_cbranch_vccz .LBB0_9", "s_branch .LBB0_1",
         ".LBB0_9:", "s_endpgm"]
    assert barriers_behind_the_sweep(parent) == 2 and lds_writes_in_the_polling_loop(parent) == [store]
    assert loop_scratch(parent) == [("scratch_load_dword", 4)]
    # this change: a select in the loop, half a tree, one barrier
    keep = "v_cndmask_b32_e32 v10, v10, v4, vcc"
    own = head + [l % keep if "%s" in l else l for l in poll] + \
        [w % 0, "ds_write_b64 v1, v[2:3]", "ds_write_b32 v1, v2", "s_barrier", "ds_read_b128 v[4:7], v1", "s_cbranch_vccz .LBB0_9",
         "s_branch .LBB0_1", ".LBB0_9:", "s_endpgm"]
    assert barriers_behind_the_sweep(own) == 1 and lds_writes_in_the_polling_loop(own) == [] and loop_scratch(own) == []
    # a barrier behind the back edge is not the exchange's
    assert barriers_behind_the_sweep(own + ["s_barrier"]) == 1
    # a reload in a block of the loop that is laid out behind the back edge is the loop's
    tail = own[:-2] + [".LBB0_7:                         ;   in Loop: Header=BB0_1 Depth=1", "scratch_load_dword v1, off, off offset:16",
                       "s_branch .LBB0_1", ".LBB0_8:                         ;   in Loop: Header=BB0_1 Depth=1",
                       "scratch_load_dword v1, off, off", ".LBB0_9:", "scratch_load_dword v1, off, off offset:32", "s_endpgm"]
    assert loop_scratch(tail) == [("scratch_load_dword", 16), ("scratch_load_dword", 0)]


def test_one_barrier_and_no_lds_store_in_the_polling_loop(isa):
    lines, spills = xb._kernel(isa["persist_k4"], 512, 1, 0, 0, 0)
    assert barriers_behind_the_sweep(lines) == 1
    assert lds_writes_in_the_polling_loop(lines) == []
    assert spills <= PARENT_SPILLS, spills
    new = [s for s in loop_scratch(lines) if s not in PARENT_LOOP_SCRATCH]
    assert not new, new


@pytest.mark.parametrize("unit", OTHER_UNITS)
def test_the_other_units_keep_the_parents_registers(isa, unit):
    golden = json.load(open(GOLDEN))[unit]
    text = isa[unit]
    got = {}
    for m in re.finditer(r"\.name:\s+(_ZN4magk12k_cg_persist\S+)\n", text):
        meta = text[m.start():]
        got[m.group(1)] = [int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)),
                           int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))]
    assert got == golden, {k: (got.get(k), golden.get(k)) for k in set(got) | set(golden) if got.get(k) != golden.get(k)}
