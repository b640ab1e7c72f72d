"""CPU: the exchange of the on-chip CG kernel issues its loads in batches IN THE EMITTED ISA.

persist_exchange (persist_kernel.h) fetches a lane's piece of the records and the q of its halo entries with 16-byte sc1
buffer loads, two per value.  With every fetch inside an `if` of its own and its result used at once, a pass of the sweep
was up to three dependent round trips through the memory side: two record loads, wait, two loads of halo entry 0, wait, two
of entry 1, wait.  Now the 2 * kPersistNh halo loads go out in front of the exchange's first wait (the two s_sleep) and
the two record loads behind it, all of them before the first `s_waitcnt vmcnt`; every further pass of the sweep has its
loads in front of its first wait in the same way.

Checked here, on the `make isa` listings, for every single-GPU instantiation of persist_shapes.h that runs on a grid (not
ONE, not MG; all four objects), in the CG loop's exchange -- the last pair of `s_sleep` of the kernel, back to the `s_barrier`
before it and on to the `s_barrier` behind it -- along the path of a wave that has all its pieces to fetch (a wave none of
whose lanes has a piece jumps over those loads: at a branch the walk goes where the loads are):

  * at the sleeps, 2 * kPersistNh `buffer_load_dwordx4 ... sc1` have been issued since the last `s_waitcnt vmcnt`;
  * the first `s_waitcnt vmcnt` behind the sleeps comes after two more: 2 + 2 * kPersistNh in flight together;
  * a further pass of the sweep has the same shape: 2 * kPersistNh loads between the last vmcnt wait and the loop's
    `s_sleep 1`, two more behind it before the next vmcnt wait;
  * no `scratch_load` between the sleeps and the barrier;
  * `.vgpr_spill_count` is not above the parent commit's.

The listing is read for those mnemonics, labels, branches and the kernels' metadata; nothing else."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "magnetite_amd", "csrc")
NH = 2  # kPersistNh: halo entries per thread

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
            if not mg and not one:
                out.append((unit, b, ebm, nptx, var, lc))
    return out


CASES = _cases()


def parent_spills(unit, b, ebm, nptx):
    """.vgpr_spill_count of the parent commit: the four-slot structured kernel of persist_k4 spills 4, every other single-GPU
    instantiation on a grid 0."""
    return 4 if unit == "persist_k4" else 0


@pytest.fixture(scope="module")
def isa():
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "isa"], stdout=subprocess.DEVNULL)
    return {u: open(os.path.join(CSRC, "build", u + ".s")).read() for u in UNITS}


def _kernel(text, b, ebm, nptx, var, lc):
    name = "_ZN4magk12k_cg_persistILi%dELb0ELi512ELi%dELb0ELi%dELb%dELb%dEEEvNS_13PersistParamsE" % (b, ebm, nptx, var, lc)
    start = text.index("\n" + name + ":")
    body = text[start:text.index("\n.Lfunc_end", start)]
    meta = text[text.index(".name:           " + name + "\n"):]
    spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
    return [l.strip() for l in body.splitlines()], spills


def _is_load(l):
    return l.startswith("buffer_load_dwordx4") and l.endswith("sc1")


def _is_vmwait(l):
    return l.startswith("s_waitcnt") and "vmcnt(" in l


def _label(l):
    m = re.match(r"(\.LBB\d+_\d+):", l)
    return m.group(1) if m else None


def _loads_ahead(lines, i):
    """Does the basic block that starts at line i hold a granule load?"""
    for l in lines[i:]:
        if _is_load(l):
            return True
        if _label(l) or l.startswith(("s_cbranch", "s_branch", "s_barrier", "s_sleep")):
            return False
    return False


def _bounds(lines):
    pair = max(i for i in range(len(lines) - 1) if lines[i].startswith("s_sleep") and lines[i + 1].startswith("s_sleep"))
    start = max(i for i in range(pair) if lines[i].startswith("s_barrier"))
    end = min(i for i in range(pair, len(lines)) if lines[i].startswith("s_barrier"))
    return start, pair, end


def walk(lines):
    """Along the path of a wave that fetches everything, from the barrier before the loop's exchange to the one behind it:
    (granule loads issued since the last vmcnt wait when the sleeps are reached, the same count at the first vmcnt wait behind
    the sleeps, the scratch_load lines between the sleeps and the barrier -- in the text, on any path)."""
    start, pair, end = _bounds(lines)
    at_sleep, count = _walk_from(lines, start, lambda i: i == pair)
    reloads = [l for l in lines[pair:end] if l.startswith("scratch_load")]
    return at_sleep, count, reloads


def walk_further_pass(lines):
    """The same two counts for a further pass of the sweep: from the first vmcnt wait behind the sleeps (on the path of a wave
    that still misses something: at `s_cbranch` the walk goes on in the text, which is where the compiler puts the loop) to the
    loop's `s_sleep 1` and on to the next vmcnt wait."""
    start, pair, end = _bounds(lines)
    sleep1 = [i for i in range(pair + 2, end) if lines[i].startswith("s_sleep")]
    assert len(sleep1) == 1, sleep1  # the sweep's own `s_sleep 1`
    back = max(i for i in range(pair, sleep1[0]) if _is_vmwait(lines[i]) or lines[i].startswith("s_sleep"))
    return _walk_from(lines, back, lambda i: i == sleep1[0])


def _walk_from(lines, start, is_sleep):
    labels = {_label(l): i for i, l in enumerate(lines) if _label(l)}
    i, count, at_sleep, steps = start + 1, 0, None, 0
    while True:
        steps += 1
        assert steps < 20000 and i < len(lines), "lost the path"
        l = lines[i]
        if is_sleep(i):
            at_sleep = count
        if _is_load(l):
            count += 1
        elif _is_vmwait(l):
            if at_sleep is not None:
                break
            count = 0
        elif l.startswith("s_barrier"):
            break
        elif l.startswith("s_branch"):
            i = labels[l.split()[1]]
            continue
        elif l.startswith("s_cbranch"):
            t = labels[l.split()[1]]
            if _loads_ahead(lines, t + 1) and not _loads_ahead(lines, i + 1):
                i = t
                continue
        i += 1
    return at_sleep, count


def test_the_walker_on_the_patterns_this_is_about():
    h, r, w = "buffer_load_dwordx4 v[0:3], v9, s[0:3], 0 offen sc1", "buffer_load_dwordx4 v[4:7], v8, s[4:7], 0 offen offset:16 sc1", "s_waitcnt vmcnt(%d)"
    tail = ["s_barrier"]
    serial = ["s_barrier", "s_sleep 6", "s_sleep 4", r, r, w % 1, w % 0, h, h, w % 0, h, h, w % 0] + tail  # the parent
    assert walk(serial)[:2] == (0, 2)
    together = ["s_barrier", "s_sleep 6", "s_sleep 4", r, r, h, h, h, h, w % 5] + tail  # everything behind the sleeps
    assert walk(together)[:2] == (0, 6)
    split = ["s_barrier", w % 0, h, h, h, h, "s_sleep 8", "s_sleep 6", r, r, w % 1] + tail  # the halo loads in front of them
    assert walk(split)[:2] == (4, 6)
    skipping = ["s_barrier", "s_cbranch_scc1 .LBB0_2", ".LBB0_1:", h, h, "s_branch .LBB0_3", ".LBB0_2:", "v_mov_b32_e32 v0, 0",
                "s_cbranch_scc0 .LBB0_1", ".LBB0_3:", "s_cbranch_scc1 .LBB0_4", h, h, ".LBB0_4:", "s_sleep 8", "s_sleep 6",
                "s_cbranch_vccnz .LBB0_5", r, r, "s_branch .LBB0_6", ".LBB0_5:", w % 0, ".LBB0_6:", w % 1,
                "scratch_load_dword v1, off, off"] + tail  # a wave without pieces jumps over the loads
    assert walk(skipping) == (4, 6, ["scratch_load_dword v1, off, off"])
    loop = ["s_barrier", h, h, h, h, "s_sleep 8", "s_sleep 6", ".LBB0_1:", r, r, w % 1, w % 0, "s_cbranch_scc1 .LBB0_2", h, h, h, h,
            "s_sleep 1", "s_branch .LBB0_1", ".LBB0_2:"] + tail
    assert walk(loop)[:2] == (4, 6) and walk_further_pass(loop) == (4, 6)
    peeled = ["s_barrier", h, h, h, h, "s_sleep 8", "s_sleep 6", r, r, w % 0, "s_cbranch_scc1 .LBB0_2", ".LBB0_1:", "s_sleep 1", r, r,
              w % 0, h, h, w % 0, h, h, w % 0, "s_cbranch_scc0 .LBB0_1", ".LBB0_2:"] + tail  # a serial loop behind a batched first pass
    assert walk(peeled)[:2] == (4, 6) and walk_further_pass(peeled) != (4, 6)


@pytest.mark.parametrize("unit,b,ebm,nptx,var,lc", CASES, ids=["%s-%d-%d-%d" % c[:4] for c in CASES])
def test_exchange_issues_its_loads_together(isa, unit, b, ebm, nptx, var, lc):
    lines, spills = _kernel(isa[unit], b, ebm, nptx, var, lc)
    at_sleep, at_wait, reloads = walk(lines)
    assert at_sleep == 2 * NH, at_sleep  # the halo loads, in front of the exchange's first wait
    assert at_wait == 2 + 2 * NH, at_wait  # ... and the record loads behind it, before the first vmcnt wait
    assert walk_further_pass(lines) == (2 * NH, 2 + 2 * NH)
    assert not reloads, reloads
    assert spills <= parent_spills(unit, b, ebm, nptx), spills
