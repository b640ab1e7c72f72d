"""CPU: csrc/persist_shapes.h states the instantiations of the on-chip CG kernel once and selects among them in one function.
tests/cpp/persist_shapes.cpp (host compiler, that header alone) prints the row lists and persist_shape's answer over a domain
that reaches every row; here the answers are held against a transcription of the five places that made the choice before the
header existed -- persist_launch's two ladders, persist_launch_general, persist_cases_shape, persist_launch_cases and
persist_launch_variants -- written from those functions, not from the header."""
import itertools

import pytest

from persist_shapes_util import compile_and_parse

SINGLE, CASES, VARIANTS = 0, 1, 2
NPT = 4  # kPersistNpt


def old_general(B, nranks, eb_mode):
    """persist_launch_general: a 12-way tree over (several ranks, eb_mode, B); anything but 256 is 512, anything but 1, 2 is 0"""
    mg = nranks > 1
    ebm = eb_mode if eb_mode in (1, 2) else 0
    return (256 if B == 256 else 512, mg, ebm, False, 0)


def old_single(B, nranks, grid, tiles_per_wg, eb_mode):
    """persist_launch"""
    if nranks == 1 and B == 512 and eb_mode != 0 and (grid == 1 or tiles_per_wg < 4):
        one = grid == 1
        npt = tiles_per_wg if 1 <= tiles_per_wg < 4 else 0
        ladder = [(e, False, n) for e in (1, 2) for n in (1, 2, 3)] + [(e, True, n) for e in (1, 2) for n in (1, 2, 3)]
        ladder += [(1, True, 0), (2, True, 0)]
        return (512, False, eb_mode, one, npt) if (eb_mode, one, npt) in ladder else None
    if nranks > 1 and B == 512 and eb_mode != 0 and 1 <= tiles_per_wg < 4:
        npt = tiles_per_wg
        return (512, True, eb_mode, False, npt) if (eb_mode, npt) in [(e, n) for e in (1, 2) for n in (1, 2, 3)] else None
    return old_general(B, nranks, eb_mode)


def old_cases_shape(B, grid, tiles_per_wg, eb_mode):
    """persist_cases_shape"""
    if B != 512 or grid < 1:
        return False
    if eb_mode == 0:
        return 1 <= tiles_per_wg <= NPT
    return 1 <= tiles_per_wg <= NPT if grid == 1 else tiles_per_wg == 1


def old_set(B, nranks, grid, tiles_per_wg, eb_mode):
    """persist_launch_cases; persist_launch_variants is the same with VAR = true"""
    if not old_cases_shape(B, grid, tiles_per_wg, eb_mode) or nranks != 1:
        return None
    if eb_mode == 0:
        return (512, False, 0, False, 0)
    one = grid == 1
    npt = tiles_per_wg if tiles_per_wg < 4 else 0
    ladder = [(False, 1), (True, 1), (True, 2), (True, 3), (True, 0)]
    return (512, False, eb_mode, one, npt) if eb_mode in (1, 2) and (one, npt) in ladder else None


def old_choice(B, nranks, grid, tiles_per_wg, eb_mode, members):
    if members == SINGLE:
        return old_single(B, nranks, grid, tiles_per_wg, eb_mode)
    return old_set(B, nranks, grid, tiles_per_wg, eb_mode)


def domain():
    for B in (256, 512):
        for nranks, grid in itertools.product((1, 2, 8), (1, 2, 3)):
            for k in range(1, (8 if B == 256 else 4) + 1):
                for eb_mode, members in itertools.product((0, 1, 2), (SINGLE, CASES, VARIANTS)):
                    yield (B, nranks, grid, k, eb_mode, members)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    return compile_and_parse(tmp_path_factory.mktemp("persist_shapes"))


def test_the_lists_have_31_1_11_and_11_distinct_rows(printed):
    rows, _ = printed
    for name, n in (("main", 31), ("k4", 1), ("cases", 11), ("variants", 11)):
        assert len(rows[name]) == n and len(set(rows[name])) == n, (name, rows[name])
    assert rows["k4"] == [(512, False, 1, False, 0)]
    assert not set(rows["main"]) & set(rows["k4"])  # every single-problem kernel in ONE object


def test_persist_shape_chooses_what_the_five_ladders_chose(printed):
    rows, shapes = printed
    inputs = list(domain())
    assert sorted(shapes) == sorted(inputs)
    chosen = {"main": set(), "k4": set(), "cases": set(), "variants": set()}
    for key in inputs:
        want, got = old_choice(*key), shapes[key]
        if want is None:
            assert got is None, (key, got)
            continue
        assert got is not None and got[0] == want and got[1] == key[5], (key, want, got)
        # ... and it is a row of the list of the object that holds it
        owner = {CASES: "cases", VARIANTS: "variants"}.get(key[5]) or ("k4" if want in rows["k4"] else "main")
        assert want in rows[owner], (key, want, owner)
        chosen[owner].add(want)
    # every row is some input's choice: nothing is instantiated that nothing selects
    for name in rows:
        assert chosen[name] == set(rows[name]), (name, set(rows[name]) - chosen[name])
    assert sum(len(v) for v in chosen.values()) == 54
