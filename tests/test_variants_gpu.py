"""GPU: V design variants of one uploaded mesh (mag_set_variants / mag_run_variants) -- other node coordinates, materials and
prescribed values on the same connectivity and mask.  A variant computes, bit for bit, what it computes as the only variant of
a call of its own; with the uploaded coordinates, bit for bit what upload + run compute; morphed, what the oracle computes on
the variant's own coordinates within the project's bars."""
import numpy as np
import pytest

from load_cases_util import make_cases
from magnetite_amd import Context, meshgen
from magnetite_amd._lib import MAG_OP_CSR
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import MESHES, MAG_TERM_MAX_ITERS, TOL_F, TOL_U, assert_case_equals, cus, rel
from variants_util import keeps_orientation, make_materials, make_shapes, make_variants, morph, variant_problem

pytestmark = pytest.mark.gpu

MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
SMALL = ("plate16", "holes3k", "frontal3k", "two_fans")
HOLES = lambda: meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3))


def solo(prob, xy, mat, u, f, i, **opts):
    """variant i as the only variant of a solve_variants call of its own"""
    pick = lambda a: None if a is None else a[i:i + 1]
    with Context(device=0, **opts) as c:
        out = c.solve_variants(prob, pick(xy), pick(mat), pick(u), pick(f))
        assert c.variants_info()["variants"] == 1
    return out[0]


def assert_oracle(out, prob, xy, mat, u, f, what):
    import oracle
    ref = oracle.run(prob.xy_flat if xy is None else xy, prob.conn_flat, prob.u_known, u, f, mat[0], mat[1], mat[2], path="sparse")
    print(what, "iterations", out["iterations"], ref["iterations"], "rel u/f/stress", rel(out["u"], ref["u"]),
          rel(out["f"], ref["f"]), rel(out["stress"], ref["stress"]))
    assert out["converged"] == 1, what
    assert abs(out["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50), what
    assert rel(out["u"], ref["u"]) <= TOL_U, what
    assert rel(out["f"], ref["f"]) <= TOL_F, what
    assert rel(out["stress"], ref["stress"]) <= TOL_F, what


@pytest.mark.parametrize("name", SMALL)
def test_variants_side_by_side_equal_their_solo_runs_bitwise(built, name):
    make, edge_blocks = MESHES[name]
    prob = make()
    with Context(device=0) as probe:  # the shape the single-case path gives this mesh
        st = probe.solve(prob)
    assert st["cg_kernel"] == 2 and st["edge_blocks"] == edge_blocks, (name, st["cg_kernel"], st["edge_blocks"])
    G = -(-st["num_tiles"] // st["tiles_per_workgroup"])
    per_launch = cus() // G
    assert per_launch >= 2, (name, G)
    V = min(2 * per_launch + 1, 300)
    xy, mat, u, f = make_variants(prob, V, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        info = c.variants_info()
    print(name, "N", prob.mesh.num_nodes, "G", G, "V", V, info, "iterations", sorted({o["iterations"] for o in outs})[:6])
    assert info == dict(variants=V, variants_per_launch=per_launch, launches=-(-V // per_launch), redone=0), info
    assert len({o["iterations"] for o in outs}) >= 2
    for o in outs:
        assert o["cg_kernel"] == 2 and o["edge_blocks"] == edge_blocks
    # the first launch's ends, the chunk boundary, the last launch
    for i in sorted({0, 1, per_launch - 1, per_launch, V - 2, V - 1}):
        assert_case_equals(outs[i], solo(prob, xy, mat, u, f, i), (name, i))


@pytest.mark.parametrize("name", SMALL)
def test_same_coordinates_equal_the_ordinary_solve_and_load_cases_bitwise(built, name):
    prob = MESHES[name][0]()
    V = 4
    mat = make_materials(prob, V, seed=3)
    u, f = make_cases(prob, V, seed=3)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, None, mat, u, f)
        assert c.variants_info()["variants_per_launch"] >= V
        plain = c.solve_variants(prob, None, None, u, f)
        cases = c.solve_cases(prob, u, f)
    for i in range(V):
        with Context(device=0) as fresh:
            ref = fresh.solve(variant_problem(prob, None, mat[i], u[i], f[i]))
        assert_case_equals(outs[i], ref, (name, "material", i))
        assert_case_equals(plain[i], cases[i], (name, "cases", i))


@pytest.mark.parametrize("name,count", [("holes3k", 3), ("frontal3k", 3), ("two_fans", 1)])
def test_morphed_variants_against_the_oracle(built, name, count):
    prob = MESHES[name][0]()
    V = count + 1
    xy, mat, u, f = make_variants(prob, V, seed=5)
    u[1], f[1] = u[0], f[0]  # (make_cases' 1e-3 x loads converge in a handful of iterations: the full loads instead)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        assert c.variants_info()["variants_per_launch"] >= V
    for i in range(1, V):  # (variant 0 keeps the uploaded shape)
        assert not np.array_equal(xy[i], xy[0])
        assert_oracle(outs[i], prob, xy[i], mat[i], u[i], f[i], (name, i))


def test_k_of_a_morphed_variant_is_the_oracle_assembly_bitwise(built):
    import oracle
    prob = MESHES["frontal3k"][0]()
    xy, mat, _, _ = make_variants(prob, 3, seed=8)
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.set_variants(xy, mat)
        rowptr, col, val = c.assemble_csr_variant(2)
        c.upload_problem(variant_problem(prob, xy[2], mat[2]))
        rowptr1, col1, val1 = c.assemble_csr()
    assert np.array_equal(rowptr, rowptr1) and np.array_equal(col, col1)
    assert np.array_equal(val, val1)  # the variants' batched assembly == the single-case assembly of that geometry
    K = oracle.assemble_sparse(xy[2], prob.conn_flat, mat[2][1], mat[2][0], mat[2][2])
    assert np.array_equal(rowptr.astype(np.int64), K.rowptr) and np.array_equal(col, K.col)
    assert np.array_equal(val, K.val)


@pytest.mark.parametrize("opts,kernel", [(dict(cg_variant=1), 1), (dict(precision=1), 4), (dict(cg_operator=MAG_OP_CSR), 3)])
def test_fallbacks_run_one_after_another(built, opts, kernel):
    prob = HOLES()
    V = 3
    xy, mat, u, f = make_variants(prob, V, seed=7)
    u[1], f[1] = u[0], f[0]
    with Context(device=0, **opts) as c:
        same = c.solve_variants(prob, None, mat, u, f)
        info = c.variants_info()
        morphed = c.solve_variants(prob, xy, mat, u, f)
    assert info == dict(variants=V, variants_per_launch=0, launches=0, redone=0), info
    for i in range(V):
        assert same[i]["cg_kernel"] == kernel and morphed[i]["cg_kernel"] == kernel
        with Context(device=0, **opts) as fresh:
            ref = fresh.solve(variant_problem(prob, None, mat[i], u[i], f[i]))
        assert_case_equals(same[i], ref, (opts, i))
        if kernel != 4:  # (the fp32 leg cannot meet the fp64 bars)
            assert_oracle(morphed[i], prob, xy[i], mat[i], u[i], f[i], (opts, i))


def test_a_mesh_of_more_than_half_the_chip_runs_its_variants_one_after_another(built):
    prob = meshgen.config_fixed_left_pull_right(meshgen.plate(320))  # 103 041 nodes: 202 tiles, one per workgroup
    V = 3
    mat = make_materials(prob, V, seed=9)
    xy = make_shapes(prob, V)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat)
        info = c.variants_info()
    assert outs[0]["num_tiles"] > cus() // 2
    assert info == dict(variants=V, variants_per_launch=0, launches=0, redone=0), info
    for out in outs:
        assert out["cg_kernel"] == 2 and out["converged"] == 1
    # variant 0 keeps the uploaded shape and material: bit for bit the ordinary solve; a morphed one: bit for bit its solo run
    with Context(device=0) as fresh:
        assert_case_equals(outs[0], fresh.solve(prob), "uploaded shape")
    assert_case_equals(outs[2], solo(prob, xy, mat, None, None, 2), "morphed")
    assert not np.array_equal(outs[2]["u"], outs[0]["u"])


def test_iteration_cap_in_one_variant_leaves_its_neighbour_alone(built):
    prob = HOLES()
    u, f = make_cases(prob, 3, seed=1)
    # variant 0: the heavy loads; variant 1: 1e-7 x the base loads on a stiffer material
    u, f = np.stack([u[2], u[0] * 1e-7]), np.stack([f[2], f[0] * 1e-7])
    mat = np.array([[prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness],
                    [2.0 * prob.youngs_modulus, 0.25, prob.part_thickness]])
    need = [solo(prob, None, mat, u, f, i)["iterations"] for i in (0, 1)]
    assert need[1] + 8 < need[0], need
    cap = ref0 = None
    for cand in range(need[1] + 2, min(need[0], need[1] + 250)):
        r = solo(prob, None, mat, u, f, 0, max_iter=cand)
        if r["termination"] == MAG_TERM_MAX_ITERS and r["best_iteration"] < r["iterations"]:
            cap, ref0 = cand, r
            break
    assert cap is not None, need
    with Context(device=0, max_iter=cap) as c:
        outs = c.solve_variants(prob, None, mat, u, f)
        info = c.variants_info()
    print("needs", need, "cap", cap, "best", ref0["best_iteration"], info)
    assert info["variants_per_launch"] >= 2 and info["launches"] == 1 and info["redone"] >= 1, info
    assert outs[0]["termination"] == MAG_TERM_MAX_ITERS and outs[0]["converged"] == 0
    assert outs[0]["best_iteration"] == ref0["best_iteration"] and outs[0]["best_param_mismatch"] == 0
    assert_case_equals(outs[0], ref0, "capped")
    assert outs[1]["converged"] == 1
    assert_case_equals(outs[1], solo(prob, None, mat, u, f, 1, max_iter=cap), "neighbour")


def test_rejection_of_a_turned_element_and_of_a_bad_material(built):
    prob = HOLES()
    V = 3
    xy, mat, u, f = make_variants(prob, V, seed=4)
    conn = prob.mesh.conn
    e = 17
    a, b, c3 = conn[e]
    p = prob.mesh.xy
    bad = xy.copy().reshape(V, -1, 2)
    bad[2, a] = p[b] + p[c3] - p[a]  # node a mirrored through the midpoint of its opposite edge: element e turns over
    bad = bad.reshape(V, -1)
    assert not keeps_orientation(prob, bad[2])
    with Context(device=0) as c:
        c.upload_problem(prob)
        with pytest.raises(MagnetiteError) as err:
            c.set_variants(bad, mat, u, f)
        assert err.value.code == MAG_ERR_BAD_ARGS
        import re
        m = re.search(r"variant (\d+), element (\d+)", str(err.value))
        assert m and int(m.group(1)) == 2, str(err.value)
        from variants_util import signed_areas
        av, a0 = signed_areas(bad[2], conn), signed_areas(p, conn)
        first = int(np.nonzero((av == 0) | ((av > 0) != (a0 > 0)))[0][0])
        assert int(m.group(2)) == first, (str(err.value), first)
        with pytest.raises(MagnetiteError) as err:  # nothing was set
            c.run_variants()
        assert err.value.code == MAG_ERR_STATE
        mat_bad = mat.copy()
        mat_bad[1, 1] = 1.0
        with pytest.raises(MagnetiteError) as err:
            c.set_variants(xy, mat_bad, u, f)
        assert err.value.code == MAG_ERR_BAD_ARGS and "variant 1" in str(err.value)
        with pytest.raises(MagnetiteError) as err:
            c.set_variants()
        assert err.value.code == MAG_ERR_BAD_ARGS


def test_state_repeat_single_case_afterwards_load_cases_kept_and_new_upload(built):
    prob = HOLES()
    V = 5
    xy, mat, u, f = make_variants(prob, V, seed=2)
    with Context(device=0) as fresh:
        ref = fresh.solve(prob)
    with Context(device=0, history_len=16) as c:
        c.upload_problem(prob)
        c.set_load_cases(u[:2], f[:2])
        c.run_cases()
        case1 = c.download_case(1)
        c.set_variants(xy, mat, u, f)
        c.run_variants()
        first = [c.download_variant(i) for i in range(V)]
        hist = c.history(8)
        c.run_variants()
        for i in range(V):
            for a, b in zip(c.download_variant(i), first[i]):
                assert np.array_equal(a, b), i
        with pytest.raises(MagnetiteError):  # the single-case results are gone after run_variants
            c.download()
        c.run()  # the upload's own problem, through the single-case path: what a fresh context computes
        for a, key in zip(c.download(), ("u", "f", "stress")):
            assert np.array_equal(a, ref[key]), key
        assert c.stats()["iterations"] == ref["iterations"]
        c.run_cases()  # the load cases set before are still there ...
        assert np.array_equal(c.download_case(1)[0], case1[0])
        c.run_variants()  # ... and so are the variants
        assert np.array_equal(c.download_variant(3)[0], first[3][0])
        c.upload_problem(prob)  # a new upload drops both sets
        for call in (c.run_variants, c.run_cases):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE
    with Context(device=0, history_len=16) as c0:  # the history is variant 0's
        c0.solve(variant_problem(prob, xy[0], mat[0], u[0], f[0]))
        assert np.array_equal(c0.history(8), hist)
