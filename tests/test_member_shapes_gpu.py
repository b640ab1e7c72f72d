"""Every member-set instantiation of the on-chip CG kernel runs in the GPU suite.  csrc/persist_shapes.h lists 11 shapes for load
cases and the same 11 for design variants; tests/test_load_cases_gpu.py's MESHES reach four of them (CITED below).  TABLE gives a
small mesh for each of the other seven -- one workgroup of two, three and four tiles with edge blocks and with overflow records,
one tile with overflow records -- and one for the triangle walk as a single workgroup per member (its shape is two_fans', its
geometry is not: grid.x == 1, two tiles, dead node slots).  On the CPU: TABLE and CITED together map onto exactly the header's
rows.  On the GPU, per mesh: load cases bit for bit against sequential solves, variants against solo runs and, with the uploaded
coordinates, against the ordinary solve and the load cases; all of them against the oracle; a repeated run gives the same bits.
A mesh that lands on another shape FAILS its tests: the single solve's and every member's stats are held against the table."""
import functools

import numpy as np
import pytest

from load_cases_util import make_cases
from magnetite_amd import Context, meshgen
from persist_shapes_util import compile_and_parse
from test_load_cases_gpu import MESHES, TOL_F, TOL_U, assert_case_equals, cus, rel, sequential
from test_persist_shapes import old_set
from test_variants_gpu import solo
from variants_util import make_materials, make_variants, variant_problem

TILE = 512


def pinched_plate24():
    """plate(24) minus two cells that leave node (9, 9) with two fans (test_load_cases_gpu.two_fans_mesh at 625 nodes): the
    whole mesh runs the triangle walk, in ONE workgroup of two tiles."""
    xy, tri, cx, cy = meshgen._grid(24, 24, 1.0, 1.0)
    keep = np.ones(cx.shape[0], dtype=bool)
    keep[[8 * 24 + 8, 9 * 24 + 9]] = False
    return meshgen._compact(xy, tri, keep, "pinched_plate24")


# name: (mesh, nodes, tiles, edge_blocks, tiles_per_workgroup, (ebm, one, nptx) of its row in MAG_PERSIST_ROWS_CASES).
# overflow_4: whether a four-tile mesh fits one workgroup's overflow pool shows only on the chip.  frontal_like(40, 0.4, 4) does
# (edge_blocks == 2, four tiles per workgroup in the single-problem path) and was taken; so do frontal_like(38, 0.4, 4), 1777
# nodes, and frontal_like(41, 0.4, 4), 2040 nodes, which were its replacements had it not.
TABLE = {
    "blocks_2": (lambda: meshgen.plate(29), 900, 2, 1, 2, (1, True, 2)),
    "blocks_3": (lambda: meshgen.plate(36), 1369, 3, 1, 3, (1, True, 3)),
    "blocks_4": (lambda: meshgen.shuffle(meshgen.plate(40), 2), 1681, 4, 1, 4, (1, True, 0)),  # (the last tile ragged)
    "overflow_1": (lambda: meshgen.frontal_like(19, 0.4, 1), 471, 1, 2, 1, (2, True, 1)),
    "overflow_2": (lambda: meshgen.frontal_like(27, 0.4, 2), 912, 2, 2, 2, (2, True, 2)),
    "overflow_3": (lambda: meshgen.frontal_like(34, 0.4, 3), 1420, 3, 2, 3, (2, True, 3)),
    "overflow_4": (lambda: meshgen.frontal_like(40, 0.4, 4), 1950, 4, 2, 4, (2, True, 0)),
    "walk_one_wg": (pinched_plate24, 625, 2, 0, 2, (0, False, 0)),
}
# the MESHES entries whose member tests (test_load_cases_gpu, test_variants_gpu) run the four other rows: name -> the row.  Above
# 2048 nodes and below one tile per CU a mesh runs one tile per workgroup (ensure_order); plate16 is one tile.
CITED = {"plate16": (1, True, 1), "holes3k": (1, False, 1), "frontal3k": (2, False, 1), "two_fans": (0, False, 0)}


@functools.lru_cache(maxsize=None)
def problem(name):
    prob = meshgen.config_fixed_left_pull_right(TABLE[name][0]())
    assert prob.mesh.num_nodes == TABLE[name][1], (name, prob.mesh.num_nodes)
    return prob


# ---------------------------------------------------------------- CPU: the accounting

def test_the_table_and_the_cited_meshes_cover_every_member_row(tmp_path):
    rows, _ = compile_and_parse(tmp_path)
    got = {}
    for name, (_, nodes, tiles, edge_blocks, k, row) in TABLE.items():
        assert problem(name).mesh.num_nodes == nodes and tiles == -(-nodes // TILE) and k == tiles <= 4, name
        got[name] = (old_set(TILE, 1, -(-tiles // k), k, edge_blocks), (TILE, False) + row)
    for name, row in CITED.items():
        nodes = MESHES[name][0]().mesh.num_nodes
        tiles = -(-nodes // TILE)
        assert tiles == 1 or 4 * TILE < nodes <= 64 * TILE, (name, nodes)  # one tile, or a grid of one tile per workgroup
        got[name] = (old_set(TILE, 1, tiles, 1, MESHES[name][1]), (TILE, False) + row)
    for name, (chosen, stated) in got.items():
        assert chosen == stated, (name, chosen, stated)
    shapes = [chosen for chosen, _ in got.values()]
    # eleven meshes for eleven rows, and walk_one_wg for the walk's second geometry
    assert sorted(shapes) == sorted(rows["cases"] + [(TILE, False, 0, False, 0)]), set(rows["cases"]) ^ set(shapes)
    assert set(shapes) == set(rows["cases"]) == set(rows["variants"])
    assert len(rows["cases"]) == len(rows["variants"]) == 11


# ---------------------------------------------------------------- GPU

def assert_shape(st, name, what):
    _, _, tiles, edge_blocks, k, _ = TABLE[name]
    got = (st["cg_kernel"], st["edge_blocks"], st["tiles_per_workgroup"], st["num_tiles"])
    assert got == (2, edge_blocks, k, tiles), (name, what, got)


def probe(name):
    """The base problem in a fresh context: it must run the table's shape.  (prob, its solution, G, members per launch)"""
    prob = problem(name)
    with Context(device=0) as c:
        out = c.solve(prob)
    assert_shape(out, name, "single")
    G = -(-out["num_tiles"] // out["tiles_per_workgroup"])
    assert G == 1, (name, G)
    per_launch = cus() // G
    assert per_launch >= 2, (name, G)
    return prob, out, G, per_launch


def line(name, prob, G, *rest):
    _, _, _, edge_blocks, k, row = TABLE[name]
    print(name, "N", prob.mesh.num_nodes, "G", G, "tiles_per_workgroup", k, "edge_blocks", edge_blocks, "row", row, *rest)


def worst(outs, refs):
    return {key: max(rel(o[key], r[key]) for o, r in zip(outs, refs)) for key in ("u", "f", "stress")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_cases_equal_sequential_solves_bitwise(built, name):
    prob, _, G, per_launch = probe(name)
    L = min(2 * per_launch + 1, 300)
    u, f = make_cases(prob, L, seed=11)
    with Context(device=0) as c:
        outs = c.solve_cases(prob, u, f)
        info = c.cases_info()
    # the first launch's ends, the chunk boundary, the last launch, and every L/24-th case
    picks = sorted(i for i in {0, 1, 2, per_launch - 1, per_launch, L - 2, L - 1} | set(range(3, L, max(1, L // 24))) if i < L)
    refs = [sequential(prob, u, f, i) for i in picks]
    line(name, prob, G, "L", L, info, "iterations", sorted({o["iterations"] for o in outs})[:6], "picks", len(picks),
         "rel to sequential", worst([outs[i] for i in picks], refs))
    assert info == dict(cases=L, cases_per_launch=per_launch, launches=-(-L // per_launch), redone=0), info
    for i, o in enumerate(outs):
        assert_shape(o, name, i)
    assert outs[0]["iterations"] != outs[1]["iterations"]  # 1e-3 x the loads: another iteration count
    for i, ref in zip(picks, refs):
        assert_shape(ref, name, ("sequential", i))
        assert_case_equals(outs[i], ref, (name, i))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_variants_equal_their_solo_runs_bitwise(built, name):
    prob, _, G, per_launch = probe(name)
    V = min(2 * per_launch + 1, 300)
    xy, mat, u, f = make_variants(prob, V, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        info = c.variants_info()
    picks = sorted(i for i in {0, 1, per_launch - 1, per_launch, V - 2, V - 1} if i < V)
    refs = [solo(prob, xy, mat, u, f, i) for i in picks]
    line(name, prob, G, "V", V, info, "iterations", sorted({o["iterations"] for o in outs})[:6],
         "rel to solo", worst([outs[i] for i in picks], refs))
    assert info == dict(variants=V, variants_per_launch=per_launch, launches=-(-V // per_launch), redone=0), info
    for i, o in enumerate(outs):
        assert_shape(o, name, i)
    assert len({o["iterations"] for o in outs}) >= 2
    for i, ref in zip(picks, refs):
        assert_shape(ref, name, ("solo", i))
        assert_case_equals(outs[i], ref, (name, i))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_uploaded_coordinates_equal_the_ordinary_solve_and_the_load_cases_bitwise(built, name):
    prob, _, G, _ = probe(name)
    V = 4
    mat = make_materials(prob, V, seed=3)
    u, f = make_cases(prob, V, seed=3)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, None, mat, u, f)
        info = c.variants_info()
        plain = c.solve_variants(prob, None, None, u, f)
        cases = c.solve_cases(prob, u, f)
    assert info == dict(variants=V, variants_per_launch=cus() // G, launches=1, redone=0), info
    refs = []
    for i in range(V):
        with Context(device=0) as fresh:
            refs.append(fresh.solve(variant_problem(prob, None, mat[i], u[i], f[i])))
    line(name, prob, G, info, "rel to the ordinary solve", worst(outs, refs), "plain variants to cases", worst(plain, cases))
    for i in range(V):
        for o in (outs[i], plain[i], cases[i], refs[i]):
            assert_shape(o, name, i)
        assert_case_equals(outs[i], refs[i], (name, "material", i))
        assert_case_equals(plain[i], cases[i], (name, "cases", i))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_single_solve_cases_and_morphed_variants_against_the_oracle(built, name):
    import oracle
    prob, single, G, _ = probe(name)
    base = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
    uc, fc = make_cases(prob, 3, seed=5)
    xy, mat, uv, fv = make_variants(prob, 4, seed=5)
    uv[1], fv[1] = uv[0], fv[0]  # (make_cases' 1e-3 x loads converge in a handful of iterations: the full loads instead)
    with Context(device=0) as c:
        cases = c.solve_cases(prob, uc, fc)
        assert c.cases_info()["cases_per_launch"] >= 3
        variants = c.solve_variants(prob, xy, mat, uv, fv)
        assert c.variants_info()["variants_per_launch"] >= 4
    todo = [("single", single, prob.xy_flat, base, prob.u_in, prob.f_in)]
    todo += [(f"case {i}", cases[i], prob.xy_flat, base, uc[i], fc[i]) for i in (0, 2)]
    for i in (1, 2, 3):  # (variant 0 keeps the uploaded shape)
        assert not np.array_equal(xy[i], xy[0])
        todo.append((f"variant {i}", variants[i], xy[i], mat[i], uv[i], fv[i]))
    for what, out, xyv, m, u, f in todo:
        ref = oracle.run(xyv, prob.conn_flat, prob.u_known, u, f, m[0], m[1], m[2], path="sparse")
        line(name, prob, G, what, "iterations", out["iterations"], ref["iterations"], "rel u/f/stress to the oracle",
             rel(out["u"], ref["u"]), rel(out["f"], ref["f"]), rel(out["stress"], ref["stress"]))
        assert_shape(out, name, what)
        assert out["converged"] == 1, (name, what)
        assert abs(out["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50), (name, what)
        assert rel(out["u"], ref["u"]) <= TOL_U, (name, what)
        assert rel(out["f"], ref["f"]) <= TOL_F, (name, what)
        assert rel(out["stress"], ref["stress"]) <= TOL_F, (name, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_a_repeated_run_gives_the_same_bits(built, name):
    prob, _, G, per_launch = probe(name)
    n = per_launch + 1  # two launches: member per_launch is the second one's first
    xy, mat, u, f = make_variants(prob, n, seed=11)
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.set_load_cases(u, f)
        c.set_variants(xy, mat, u, f)
        for run, download, stats, info in ((c.run_cases, c.download_case, c.case_stats, c.cases_info),
                                           (c.run_variants, c.download_variant, c.variant_stats, c.variants_info)):
            run()
            first = [(download(i), stats(i)) for i in (0, per_launch)]
            assert list(info().values()) == [n, per_launch, 2, 0], info()
            run()
            assert list(info().values()) == [n, per_launch, 2, 0], info()
            for i, (arrays, st) in zip((0, per_launch), first):
                again, st2 = download(i), stats(i)
                assert_shape(st, name, i)
                assert_shape(st2, name, i)
                assert st2["iterations"] == st["iterations"], (name, run.__name__, i)
                for a, b, key in zip(again, arrays, ("u", "f", "stress")):
                    assert np.array_equal(a, b), (name, run.__name__, i, key, rel(a, b))
            line(name, prob, G, run.__name__, "twice", info(), "iterations", [st["iterations"] for _, st in first])
