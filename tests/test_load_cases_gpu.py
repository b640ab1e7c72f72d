"""GPU: L load cases on one uploaded mesh (mag_set_load_cases / mag_run_cases) give, case by case and BIT FOR BIT, what a
sequential upload + run of that case gives -- whether the CG solves ran side by side in launches of the on-chip load-case
kernel or one after another through the single-case phases -- and the launches are chunked as documented."""
import functools
import subprocess
import sys

import numpy as np
import pytest

from load_cases_util import case_problem, make_cases
from magnetite_amd import Context, meshgen
from magnetite_amd._lib import MAG_OP_CSR

pytestmark = pytest.mark.gpu

MAG_ERR_STATE = 7
MAG_TERM_MAX_ITERS = 2
TOL_U, TOL_F = 1e-8, 1e-7  # the project's parity bars (tests/test_gpu_parity.py)
BITWISE_STATS = ("iterations", "cg_kernel", "edge_blocks", "tiles_per_workgroup", "converged", "termination",
                 "best_iteration", "n_free")


@functools.lru_cache(maxsize=None)
def cus():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process: torch brings a HIP runtime of
    its own, which finds no GPU in a process where the library's has already opened it."""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.split()[-1])


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def two_fans_mesh():
    """plate(64) minus two cells that leave node (21, 21) with two fans (as tests/test_gpu_parity.py builds it): the whole
    mesh then runs the triangle walk."""
    xy, tri, cx, cy = meshgen._grid(64, 64, 1.0, 1.0)
    keep = np.ones(cx.shape[0], dtype=bool)
    keep[[20 * 64 + 20, 21 * 64 + 21]] = False
    return meshgen._compact(xy, tri, keep, "pinched_plate")


def sequential(prob, u, f, i, **opts):
    with Context(device=0, **opts) as c:
        return c.solve(case_problem(prob, u[i], f[i]))


def assert_case_equals(out, ref, what):
    for key in ("u", "f", "stress"):
        assert np.array_equal(out[key], ref[key]), (what, key, rel(out[key], ref[key]))
    for key in BITWISE_STATS:
        assert out[key] == ref[key], (what, key, out[key], ref[key])
    assert np.float64(out["final_cost"]).tobytes() == np.float64(ref["final_cost"]).tobytes(), what
    assert np.float64(out["rhs_norm"]).tobytes() == np.float64(ref["rhs_norm"]).tobytes(), what


MESHES = {
    "plate16": (lambda: meshgen.config_fixed_left_pull_right(meshgen.plate(16)), 1),
    "holes3k": (lambda: meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3)), 1),
    "frontal3k": (lambda: meshgen.config_fixed_left_pull_right(meshgen.frontal_like(52, 0.4, 2)), 2),
    "two_fans": (lambda: meshgen.config_fixed_left_pull_right(two_fans_mesh()), 0),
    "plate100k": (lambda: meshgen.baseline_problem("plate100k"), 1),
}


@pytest.mark.parametrize("name", list(MESHES))
def test_cases_equal_sequential_solves_bitwise_one_launch_per_chunk(built, name):
    make, edge_blocks = MESHES[name]
    prob = make()
    with Context(device=0) as probe:  # the shape the single-case path gives this mesh
        st = probe.solve(prob)
    assert st["cg_kernel"] == 2 and st["edge_blocks"] == edge_blocks, (name, st["cg_kernel"], st["edge_blocks"])
    G = -(-st["num_tiles"] // st["tiles_per_workgroup"])
    per_launch = cus() // G
    assert per_launch >= 2, (name, G)
    L = min(2 * per_launch + 1, 300)
    u, f = make_cases(prob, L, seed=11)
    with Context(device=0) as c:
        outs = c.solve_cases(prob, u, f)
        info = c.cases_info()
    print(name, "N", prob.mesh.num_nodes, "G", G, "L", L, info, "iterations", sorted({o["iterations"] for o in outs})[:6])
    assert info == dict(cases=L, cases_per_launch=per_launch, launches=-(-L // per_launch), redone=0), info
    assert outs[0]["iterations"] != outs[1]["iterations"]  # 1e-3 x the loads: another iteration count
    # every case of the first launch's ends and of the last launch; for the small meshes, all of them
    picks = range(L) if prob.mesh.num_nodes < 20000 and L <= 120 else sorted({0, 1, 2, per_launch - 1, per_launch, L - 2, L - 1} | set(range(3, L, max(1, L // 24))))
    for i in picks:
        assert_case_equals(outs[i], sequential(prob, u, f, i), (name, i))


def test_cases_against_the_oracle(built):
    import oracle
    prob = meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3))
    u, f = make_cases(prob, 3, seed=5)
    with Context(device=0) as c:
        outs = c.solve_cases(prob, u, f)
        assert c.cases_info()["cases_per_launch"] >= 3
    for i, out in enumerate(outs):
        ref = oracle.run(prob.xy_flat, prob.conn_flat, prob.u_known, u[i], f[i], prob.youngs_modulus, prob.poisson_ratio,
                         prob.part_thickness, path="sparse")
        print("case", i, "iterations", out["iterations"], ref["iterations"], "rel u/f/stress", rel(out["u"], ref["u"]),
              rel(out["f"], ref["f"]), rel(out["stress"], ref["stress"]))
        assert out["converged"] == 1
        assert abs(out["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50), i
        assert rel(out["u"], ref["u"]) <= TOL_U, i
        assert rel(out["f"], ref["f"]) <= TOL_F, i
        assert rel(out["stress"], ref["stress"]) <= TOL_F, i


@pytest.mark.parametrize("opts,kernel", [(dict(cg_variant=1), 1), (dict(precision=1), 4), (dict(cg_operator=MAG_OP_CSR), 3)])
def test_fallbacks_give_the_sequential_numbers(built, opts, kernel):
    prob = meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3))
    u, f = make_cases(prob, 3, seed=7)
    with Context(device=0, **opts) as c:
        outs = c.solve_cases(prob, u, f)
        info = c.cases_info()
    assert info == dict(cases=3, cases_per_launch=0, launches=0, redone=0), info
    for i, out in enumerate(outs):
        assert out["cg_kernel"] == kernel
        assert_case_equals(out, sequential(prob, u, f, i, **opts), (opts, i))


def test_a_mesh_of_more_than_half_the_chip_runs_its_cases_one_after_another(built):
    prob = meshgen.config_fixed_left_pull_right(meshgen.plate(320))  # 103 041 nodes: 202 tiles, one per workgroup
    u, f = make_cases(prob, 3, seed=9)
    with Context(device=0) as c:
        outs = c.solve_cases(prob, u, f)
        info = c.cases_info()
    assert outs[0]["num_tiles"] > cus() // 2
    assert info == dict(cases=3, cases_per_launch=0, launches=0, redone=0), info
    for i, out in enumerate(outs):
        assert out["cg_kernel"] == 2
        assert_case_equals(out, sequential(prob, u, f, i), i)


def test_iteration_cap_in_one_case_leaves_its_neighbour_alone(built):
    prob = meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3))
    u, f = make_cases(prob, 3, seed=1)
    # case 0: scaled loads plus random nodal forces; case 1: 1e-7 x the base loads -- under the absolute stop rule it needs
    # a fraction of case 0's iterations, which leaves the early, non-monotone part of case 0's residual history for the cap
    u, f = np.stack([u[2], u[0] * 1e-7]), np.stack([f[2], f[0] * 1e-7])
    need = [sequential(prob, u, f, i)["iterations"] for i in (0, 1)]
    assert need[1] + 8 < need[0], need
    # a cap between the two needs at which plain CG's best iterate is not its last one (its residual norm is not monotone):
    # only then is there a best_param to recover, i.e. a case to redo
    cap = ref0 = None
    for cand in range(need[1] + 2, min(need[0], need[1] + 250)):
        r = sequential(prob, u, f, 0, max_iter=cand)
        if r["termination"] == MAG_TERM_MAX_ITERS and r["best_iteration"] < r["iterations"]:
            cap, ref0 = cand, r
            break
    assert cap is not None, need
    with Context(device=0, max_iter=cap) as c:
        outs = c.solve_cases(prob, u, f)
        info = c.cases_info()
    print("needs", need, "cap", cap, "best", ref0["best_iteration"], info)
    assert info["cases_per_launch"] >= 2 and info["launches"] == 1 and info["redone"] >= 1, info
    assert outs[0]["termination"] == MAG_TERM_MAX_ITERS and outs[0]["converged"] == 0
    assert outs[0]["best_iteration"] == ref0["best_iteration"] and outs[0]["best_param_mismatch"] == 0
    assert_case_equals(outs[0], ref0, "capped")
    assert outs[1]["converged"] == 1
    assert_case_equals(outs[1], sequential(prob, u, f, 1, max_iter=cap), "neighbour")


def test_state_repeat_single_case_afterwards_and_new_upload(built):
    from magnetite_amd.solver import MagnetiteError
    prob = meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3))
    u, f = make_cases(prob, 5, seed=2)
    with Context(device=0) as fresh:
        ref = fresh.solve(prob)
    with Context(device=0, history_len=16) as c:
        first = c.solve_cases(prob, u, f)
        hist = c.history(8)
        c.run_cases()
        for i in range(5):
            again = c.download_case(i)
            for a, key in zip(again, ("u", "f", "stress")):
                assert np.array_equal(a, first[i][key]), (i, key)
            assert c.case_stats(i)["iterations"] == first[i]["iterations"]
        with pytest.raises(MagnetiteError):  # the single-case results are gone after run_cases
            c.download()
        c.run()  # the upload's own loads, through the single-case path: what a fresh context computes
        got = c.download()
        for a, key in zip(got, ("u", "f", "stress")):
            assert np.array_equal(a, ref[key]), key
        assert c.stats()["iterations"] == ref["iterations"]
        c.run_cases()  # ... and the cases are still there
        assert np.array_equal(c.download_case(3)[0], first[3]["u"])
        c.upload_problem(prob)  # a new upload drops them
        with pytest.raises(MagnetiteError) as e:
            c.run_cases()
        assert e.value.code == MAG_ERR_STATE
    with Context(device=0, history_len=16) as c0:  # the history is case 0's
        c0.solve(case_problem(prob, u[0], f[0]))
        assert np.array_equal(c0.history(8), hist)
