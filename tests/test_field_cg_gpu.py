"""mag_options.field_cg on the device: the fused CG over the assembled K's block rows (k_cg_field, cg_kernel 5) under an element
stiffness field, against the numpy twin (tests/field_cg_ref.py), the direct solve and the CSR operator's phase it replaces."""
import functools
import math
import os

import numpy as np
import pytest

import adjoint_ref as aref
import design_ref as dref
import field_cg_ref as fref
from load_cases_util import case_problem, make_cases
from magnetite_amd import Context
from magnetite_amd._lib import MAG_STOP_REL, MAG_TERM_MAX_ITERS
from magnetite_amd.solver import MagnetiteError
from test_adjoint_gpu import assert_parity
from test_design_gpu import solver_spread
from test_load_cases_gpu import TOL_F, assert_case_equals, rel

pytestmark = pytest.mark.gpu

MAG_ERR_STATE = 7
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = [1, 2, 3]
TOL = 1e-12
BITWISE = ("u", "f", "stress")


def run_field(prob, scale, **opts):
    """upload + set_element_scale + run: dict(u, f, stress, **stats)"""
    with Context(device=0, **opts) as c:
        c.upload_problem(prob)
        c.set_element_scale(scale)
        c.run()
        return dict(zip(BITWISE, c.download()), **c.stats())


def same_bits(a, b, what):
    for k in BITWISE:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["iterations"] == b["iterations"] and np.float64(a["final_cost"]).tobytes() == np.float64(b["final_cost"]).tobytes(), what


def assert_solve_bars(out, prob, sol, what, tol=TOL, factor=1.0):
    """the bars of test_the_solve_under_a_field (tests/test_design_gpu.py), derived there"""
    u, f, free = out["u"], out["f"], sol["free"]
    nb = np.linalg.norm(sol["b"])
    residual = np.linalg.norm(sol["Kff"] @ u[free] - sol["b"])
    print(what, "kernel", out["cg_kernel"], "iterations", out["iterations"], "residual / |b|", residual / nb, "rel u", rel(u, sol["u"]),
          "bar", sol["cond"] * 10 * tol)
    assert out["converged"] == 1, what
    assert residual <= factor * 10 * tol * nb, what
    assert rel(u, sol["u"]) <= factor * sol["cond"] * 10 * tol, what
    for d in (0, 1):
        applied = float(np.sum(prob.f_in[d::2][prob.u_known[d::2] == 0]))
        reactions = float(np.sum(f[d::2][prob.u_known[d::2] == 1]))
        assert abs(reactions + applied) <= factor * math.sqrt(free.size) * 10 * tol * nb + 2.0 ** -40 * np.abs(f[d::2]).sum(), (what, d)
    assert rel(f, sol["f"]) <= TOL_F, what


# ---- the solve
SOLVES = [
    ("plate_6x5", "pull", "random"), ("plate_6x5", "rollers", "two-phase"), ("frontal16", "pull", "two-phase"),
    ("frontal16", "rollers", "random"), ("frontal32s", "pull", "random"), ("frontal32s", "rollers", "two-phase"),
    ("plate_40x24", "pull", "two-phase"), ("plate_40x24", "rollers", "random"), ("plate_40x24", "cantilever", "ones"),
    ("frontal16", "pull", "ones"),
]


@pytest.mark.parametrize("grid", [None, "2"])
@pytest.mark.parametrize("tile", [256, 512])
@pytest.mark.parametrize("name,bc,which", SOLVES)
def test_the_solve_on_the_block_rows(built, monkeypatch, name, bc, which, tile, grid):
    """MAG_STOP_REL, tol = 1e-12, field_cg 1, 2 and 3: cg_kernel 5, converged, the true residual under the twin's K_ff, u against
    the direct solve, the reactions in equilibrium -- with one tile and several, every workgroup walking one tile or several"""
    if grid:
        monkeypatch.setenv("MAG_TUNE_GRID", grid)
    prob, sol, s = fref.problem(name, bc), fref.direct(name, bc, which), fref.field(name, which)
    for kind in KINDS:
        out = run_field(prob, s, stop_mode=MAG_STOP_REL, tol=TOL, tile_nodes=tile, field_cg=kind)
        assert out["cg_kernel"] == 5 and out["lds_operator"] == 1, (kind, out["cg_kernel"])
        assert_solve_bars(out, prob, sol, (name, bc, which, tile, grid, kind))


# ---- the operator and the recurrence
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["random", "two-phase"])
@pytest.mark.parametrize("name", ["frontal16", "frontal32s"])
def test_the_history_starts_on_the_twins(built, name, which, kind):
    """the project's PCG bars (test_preconditioned_cg_matches_oracle_pcg): the first 15 costs within rtol 1e-9 of the twin's --
    same operator, same fp32 inverse blocks, same recurrence --, the iteration count within max(5, ref // 20)"""
    n = 15
    prob, s = fref.problem(name, "rollers"), fref.field(name, which)
    ref = fref.twin_run(name, "rollers", which, kind, 1e-10, n)
    with Context(device=0, stop_mode=MAG_STOP_REL, tol=1e-10, tile_nodes=256, field_cg=kind, history_len=n) as c:
        c.upload_problem(prob)
        c.set_element_scale(s)
        c.run()
        hist, st = c.history(n), c.stats()
    print(name, which, kind, "iterations", st["iterations"], "twin", ref["iterations"], "history", np.max(np.abs(hist / ref["history"][:n] - 1)))
    assert st["cg_kernel"] == 5 and st["converged"] == 1 and st["num_tiles"] == (2 if name == "frontal16" else 5)
    assert np.allclose(hist, ref["history"][:n], rtol=1e-9), np.max(np.abs(hist / ref["history"][:n] - 1))
    assert abs(st["iterations"] - ref["iterations"]) <= max(5, ref["iterations"] // 20)


def test_the_preconditioner_earns_its_place(built):
    """shuffled frontal32 under the two-phase field at a relative 1e-8: Jacobi and block-Jacobi need at most 0.75 of plain CG's
    iterations (numpy, exact inverses, the same mesh unshuffled: 1 285, 778 and 711 -- ratios 0.61 and 0.55)"""
    prob, s = fref.problem("frontal32s", "pull"), fref.field("frontal32s", "two-phase")
    its = {k: run_field(prob, s, stop_mode=MAG_STOP_REL, tol=1e-8, tile_nodes=256, field_cg=k)["iterations"] for k in KINDS}
    print("iterations", its)
    assert its[2] <= 0.75 * its[1] and its[3] <= 0.75 * its[1]


# ---- same answer as the phase it replaces
@pytest.mark.parametrize("name,bc,which", [("frontal16", "rollers", "two-phase"), ("frontal32s", "pull", "random")])
def test_the_same_answer_as_the_csr_phase(built, name, bc, which):
    prob, sol, s = fref.problem(name, bc), fref.direct(name, bc, which), fref.field(name, which)
    base = run_field(prob, s, stop_mode=MAG_STOP_REL, tol=TOL, tile_nodes=256)
    assert base["cg_kernel"] == 3
    bar = 2 * sol["cond"] * 10 * TOL
    for kind in KINDS:
        out = run_field(prob, s, stop_mode=MAG_STOP_REL, tol=TOL, tile_nodes=256, field_cg=kind)
        assert out["cg_kernel"] == 5
        print(name, kind, {k: rel(out[k], base[k]) for k in BITWISE}, "bar", bar, "iterations", out["iterations"], base["iterations"])
        for k in BITWISE:
            assert rel(out[k], base[k]) <= bar, (kind, k)
        if kind == 1:
            assert abs(out["iterations"] - base["iterations"]) <= max(5, base["iterations"] // 20)


# ---- reproducibility
@pytest.mark.parametrize("kind", KINDS)
def test_a_repeat_and_a_fresh_context_give_the_same_bits(built, monkeypatch, kind):
    name, bc, which = "frontal32s", "rollers", "two-phase"
    prob, sol, s = fref.problem(name, bc), fref.direct(name, bc, which), fref.field(name, which)
    opts = dict(stop_mode=MAG_STOP_REL, tol=TOL, tile_nodes=256, field_cg=kind)
    with Context(device=0, **opts) as c:
        c.upload_problem(prob)
        c.set_element_scale(s)
        c.run()
        first = dict(zip(BITWISE, c.download()), **c.stats())
        c.run()
        again = dict(zip(BITWISE, c.download()), **c.stats())
    fresh = run_field(prob, s, **opts)
    same_bits(first, again, "repeat")
    same_bits(first, fresh, "fresh context")
    monkeypatch.setenv("MAG_TUNE_GRID", "2")  # another summation order of the dots: other bits allowed, the bars hold
    assert_solve_bars(run_field(prob, s, **opts), prob, sol, ("grid 2", kind))


# ---- termination
@pytest.mark.parametrize("kind", KINDS)
def test_the_iteration_cap_returns_the_best_iterate(built, kind):
    prob, s = fref.problem("frontal16", "pull"), fref.field("frontal16", "random")
    opts = dict(stop_mode=MAG_STOP_REL, tol=TOL, tile_nodes=256, field_cg=kind)
    capped = run_field(prob, s, max_iter=7, **opts)
    assert capped["termination"] == MAG_TERM_MAX_ITERS and capped["converged"] == 0 and capped["cg_kernel"] == 5
    assert 1 <= capped["best_iteration"] <= 7 and capped["best_param_mismatch"] == 0
    at_best = run_field(prob, s, max_iter=capped["best_iteration"], **opts)
    for k in BITWISE:
        assert np.array_equal(capped[k], at_best[k]), k


def test_nothing_to_solve_takes_no_iteration(built):
    base = fref.problem("plate_6x5", "pull")
    prob = case_problem(base, np.zeros_like(base.u_in), np.zeros_like(base.f_in))
    out = run_field(prob, fref.field("plate_6x5", "random"), stop_mode=MAG_STOP_REL, tol=TOL, field_cg=3)
    assert out["iterations"] == 0 and out["converged"] == 1 and out["cg_kernel"] == 5 and not out["u"].any()


# ---- through the driver
def test_load_cases_equal_their_own_runs_bitwise(built):
    name = "frontal16"
    prob, s = fref.problem(name, "pull"), fref.field(name, "random")
    u_in, f_in = make_cases(prob, 3, seed=2)
    opts = dict(tile_nodes=256, field_cg=3)
    with Context(device=0, **opts) as c:
        c.upload_problem(prob)
        c.set_element_scale(s)
        c.set_load_cases(u_in, f_in)
        c.run_cases()
        assert c.cases_info()["cases_per_launch"] == 0
        outs = c._collect(3, c.download_case, c.case_stats)
    for i in range(3):
        got = run_field(case_problem(prob, u_in[i], f_in[i]), s, **opts)
        assert got["cg_kernel"] == 5 and outs[i]["cg_kernel"] == 5
        assert_case_equals(outs[i], got, ("case", i))


def test_the_adjoint_runs_on_the_block_rows(built):
    name = "frontal16"
    prob, s, sol = fref.problem(name, "pull"), fref.field(name, "random"), fref.direct(name, "pull", "random")
    w = aref.patch_weights(prob)
    with Context(device=0, stop_mode=MAG_STOP_REL, tol=TOL, tile_nodes=256, field_cg=3) as c:
        c.upload_problem(prob)
        c.set_element_scale(s)
        c.run()
        u = c.download()[0]
        adj = c.adjoint(aref.dJ1(w, u))[0]
        assert c.stats()["cg_kernel"] == 5 and c.adjoint_stats("run", 0)["cg_kernel"] == 5
    want = dref.adjoint(prob, sol["u"], aref.dJ1(w, sol["u"]), s)
    want.update(E=prob.youngs_modulus, t=prob.part_thickness)
    assert_parity(name, adj, want)
    assert rel(adj["delem"] / s, want["delem"] / s) <= 2 * TOL_F


# ---- design loop
def test_topopt_on_the_block_rows(built):
    """Context.topopt as tests/test_design_gpu.py::test_topopt_end_to_end runs it, field_cg = 3: its bars, cg_kernel 5 throughout,
    the symbolic work -- the block-row table included -- done once"""
    name = "plate_32x16"
    prob = dref.cantilever(dref.TOPOPT_MESHES[name]())
    with Context(device=0, stop_mode=MAG_STOP_REL, tol=1e-10, field_cg=3) as c:
        out = c.topopt(prob, iters=20)
    hist = out["history"]
    J = np.array([h["J"] for h in hist])
    Jref = np.array([h["J"] for h in dref.reference_trajectory(name)["history"]])
    spread = solver_spread(name)
    print("J19/J0", J[-1] / J[0], "largest relative difference to the twin", (np.abs(J - Jref) / Jref).max(), "spread", spread,
          "iterations", [h["iterations"] for h in hist])
    assert len(hist) == 20 and (J[1:] <= J[:-1]).all()
    for k, h in enumerate(hist):
        assert abs(h["volume_fraction"] - 0.5) <= 1e-10 and h["cg_kernel"] == 5, k
        if k > 0:
            assert h["ms_order"] == 0.0 and h["ms_csr_symbolic"] == 0.0, k
    assert hist[0]["ms_order"] > 0.0 and hist[0]["ms_csr_symbolic"] > 0.0
    assert (np.abs(J - Jref) <= 100 * spread * Jref).all()


# ---- off means off
def test_without_a_field_the_option_changes_no_bit(built):
    g = np.load(os.path.join(GOLD, "plate_6_5_default_bits.npz"))
    with Context(device=0, field_cg=3) as c:
        out = c.solve(fref.problem("plate_6x5", "pull"))
        rowptr, col, val = c.assemble_csr()
    for key, got in (("val", val), ("u", out["u"]), ("f", out["f"]), ("stress", out["stress"]), ("rowptr", rowptr), ("col", col)):
        assert np.array_equal(got, g[key]), key
    assert out["iterations"] == int(g["iterations"]) and out["cg_kernel"] == int(g["cg_kernel"])


def test_zero_is_the_csr_phase_and_clearing_the_field_leaves_the_kernel(built):
    name = "frontal16"
    prob, s = fref.problem(name, "pull"), fref.field(name, "random")
    without = run_field(prob, s, tile_nodes=256)
    zero = run_field(prob, s, tile_nodes=256, field_cg=0)
    odd = run_field(prob, s, tile_nodes=256, field_cg=9)  # out of range reads 0
    assert without["cg_kernel"] == zero["cg_kernel"] == odd["cg_kernel"] == 3
    same_bits(zero, without, "field_cg 0")
    same_bits(odd, without, "field_cg 9")
    with Context(device=0, tile_nodes=256) as c:
        plain = c.solve(prob)
    with Context(device=0, tile_nodes=256, field_cg=2) as c:
        c.upload_problem(prob)
        c.set_element_scale(s)
        c.run()
        assert c.stats()["cg_kernel"] == 5
        c.set_element_scale(None)
        c.run()
        cleared = dict(zip(BITWISE, c.download()), **c.stats())
        c.set_element_scale(s)
        c.run()
        assert c.stats()["cg_kernel"] == 5
        c.upload_problem(prob)
        c.run()
        uploaded = dict(zip(BITWISE, c.download()), **c.stats())
    for got in (cleared, uploaded):
        assert got["cg_kernel"] == plain["cg_kernel"] != 5
        same_bits(got, plain, "back on the non-field kernel")


# ---- fall-back and refusals
def test_without_tile_local_tables_the_csr_phase_runs(built):
    name, bc, which = "frontal16", "rollers", "random"
    prob, sol, s = fref.problem(name, bc), fref.direct(name, bc, which), fref.field(name, which)
    out = run_field(prob, s, stop_mode=MAG_STOP_REL, tol=TOL, op_variant=1, field_cg=1)
    assert out["cg_kernel"] == 3 and out["lds_operator"] == 0
    assert_solve_bars(out, prob, sol, "op_variant 1")


def test_the_preconditioner_option_still_refuses_a_field(built):
    prob = fref.problem("plate_6x5", "pull")
    with Context(device=0, preconditioner=1, cg_variant=1, field_cg=3) as c:
        c.upload_problem(prob)
        with pytest.raises(MagnetiteError, match="element stiffness field") as e:
            c.set_element_scale(np.ones(prob.mesh.num_elements))
        assert e.value.code == MAG_ERR_STATE
