"""GPU: mag_run_sensitivities -- element energies, node gradients and the scalar objective terms of solved runs, load cases and
design variants -- against the reference module applied to the ORACLE's solution; batched members bit for bit their solo runs;
the gradient against the finite differences a user would take with variants; and nothing else of the context changes."""
import numpy as np
import pytest

import sensitivities_ref as ref
from load_cases_util import case_problem, make_cases
from magnetite_amd import Context, meshgen
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import MESHES, TOL_F, assert_case_equals, rel
from test_sensitivities import base_problem
from variants_util import make_variants, variant_problem

pytestmark = pytest.mark.gpu

MAG_ERR_STATE = 7
PARITY = dict(MESHES)
del PARITY["plate100k"]
PARITY["clockwise"] = (lambda: meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24))), 1)
SCALARS = ref.SCALARS


def assert_same_bits(a, b, what):
    assert np.array_equal(a["energy"], b["energy"]), (what, "energy")
    assert np.array_equal(a["dxy"], b["dxy"]), (what, "dxy")
    for k in SCALARS:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k, a[k], b[k])


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_reference_on_the_oracles_solution(built, name):
    """rel-L2 <= 2 TOL_F for energy and dxy, relative 2 TOL_F for the scalars: the quantities are quadratic in the strains, and
    the project's bar on strain-linear outputs (f, stress) is TOL_F."""
    import oracle
    prob = PARITY[name][0]()
    with Context(device=0) as c:
        c.solve(prob)
        got = c.sensitivities("run")
    assert len(got) == 1
    got = got[0]
    sol = oracle.run(prob.xy_flat, prob.conn_flat, prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio,
                     prob.part_thickness, path="sparse")
    want = ref.of_solution(prob, sol)
    print(name, "N", prob.mesh.num_nodes, "rel energy", rel(got["energy"], want["energy"]), "rel dxy", rel(got["dxy"], want["dxy"]),
          {k: (got[k], want[k]) for k in SCALARS})
    assert rel(got["energy"], want["energy"]) <= 2 * TOL_F
    assert rel(got["dxy"], want["dxy"]) <= 2 * TOL_F
    for k in SCALARS:
        assert abs(got[k] - want[k]) <= 2 * TOL_F * abs(want[k]), (k, got[k], want[k])
    if name == "clockwise":
        assert (got["energy"] <= 0).all() and got["strain_energy"] < 0  # the signed area's sign, as K_e has it


def test_batched_members_equal_their_solo_runs_bitwise(built, monkeypatch):
    monkeypatch.setenv("MAG_TUNE_SENS_CHUNK", "3")
    prob = MESHES["holes3k"][0]()
    V = 7
    xy, mat, u, f = make_variants(prob, V, seed=11)
    with Context(device=0) as c:
        c.solve_variants(prob, xy, mat, u, f)
        outs = c.sensitivities("variants")
        again = c.sensitivities("variants")
        cases = c.solve_cases(prob, u, f)
        case_sens = c.sensitivities("cases")
    assert len(outs) == V and len(case_sens) == V
    for i in range(V):
        assert_same_bits(outs[i], again[i], ("repeat", i))
    assert len({o["strain_energy"] for o in outs}) == V
    for i in (0, 2, 3, 6):  # a chunk's first and last member, the last chunk's only one
        with Context(device=0) as solo:
            solo.solve_variants(prob, xy[i:i + 1], mat[i:i + 1], u[i:i + 1], f[i:i + 1])
            assert_same_bits(outs[i], solo.sensitivities("variants")[0], ("solo", i))
    with Context(device=0) as fresh:  # variant 0 keeps the uploaded coordinates
        assert np.array_equal(xy[0], prob.xy_flat)
        fresh.solve(variant_problem(prob, None, mat[0], u[0], f[0]))
        assert_same_bits(outs[0], fresh.sensitivities("run")[0], "uploaded coordinates")
    for i in (0, 1, 4, 6):
        with Context(device=0) as seq:
            out = seq.solve(case_problem(prob, u[i], f[i]))
            assert_case_equals(cases[i], out, ("case", i))
            assert_same_bits(case_sens[i], seq.sensitivities("run")[0], ("case", i))


@pytest.mark.parametrize("name", ["plate16", "holes3k", "frontal3k", "two_fans"])
def test_tile_staging_and_the_gather_from_memory_give_the_same_bits(built, monkeypatch, name):
    """The node kernel on the LDS image of a tile, and the one that meshes with tiles too large for the LDS fall back to."""
    prob = MESHES[name][0]()
    xy, mat, u, f = make_variants(prob, 2, seed=11)
    with Context(device=0) as c:
        c.solve_variants(prob, xy, mat, u, f)
        staged = c.sensitivities("variants")
        monkeypatch.setenv("MAG_TUNE_SENS_STAGE", "0")
        plain = c.sensitivities("variants")
    for i in range(2):
        assert np.abs(staged[i]["dxy"]).max() > 0
        assert_same_bits(staged[i], plain[i], (name, i))


def test_the_users_loop_finite_differences_through_variants(built):
    """4 x 12 variants that move one coordinate by +-h and +-h/2: Pi from the returned scalars; the base variant's dxy meets the
    inequality of the CPU test against these differences."""
    prob = base_problem(meshgen.config_fixed_left_pull_right)
    base = prob.xy_flat
    h = 1e-3 * 0.1
    rng = np.random.default_rng(2)
    dofs = rng.choice(base.size, 12, replace=False)
    xy = [base]
    for dof in dofs:
        for s in (h, -h, h / 2, -h / 2):
            v = base.copy()
            v[dof] += s
            xy.append(v)
    with Context(device=0) as c:
        c.solve_variants(prob, np.stack(xy))
        outs = c.sensitivities("variants")
    g = outs[0]["dxy"]
    gmax = np.abs(g).max()
    pi = [o["potential_energy"] for o in outs]
    for k, dof in enumerate(dofs):
        a = pi[1 + 4 * k:5 + 4 * k]
        fd_h, fd_h2 = (a[0] - a[1]) / (2 * h), (a[2] - a[3]) / h
        err, rich = abs(g[dof] - fd_h2), abs(fd_h - fd_h2)
        print("dof", dof, "g", g[dof], "err/max|g|", err / gmax, "richardson/max|g|", rich / gmax)
        assert err <= 4 * rich + 2e-7 * gmax, dof


def test_it_leaves_everything_else_alone(built):
    prob = MESHES["holes3k"][0]()
    V = 3
    xy, mat, u, f = make_variants(prob, V, seed=4)
    with Context(device=0) as plain:
        plain.solve_variants(prob, xy, mat, u, f)
        want = [(plain.download_variant(i), plain.variant_stats(i)) for i in range(V)]
        want_solve = plain.solve(prob)
    with Context(device=0) as c:
        c.solve_variants(prob, xy, mat, u, f)
        c.sensitivities("variants")
        for i in range(V):
            for a, b in zip(c.download_variant(i), want[i][0]):
                assert np.array_equal(a, b), i
            st = c.variant_stats(i)
            for k, v in want[i][1].items():
                if not k.startswith("ms_"):
                    assert st[k] == v, (i, k)
        c.run_variants()  # a new run of the set drops its sensitivities
        with pytest.raises(MagnetiteError) as e:
            c.download_sensitivity("variants", 0)
        assert e.value.code == MAG_ERR_STATE
        c.sensitivities("variants")
        c.download_sensitivity("variants", V - 1)
        with pytest.raises(MagnetiteError):
            c.download_sensitivity("variants", V)
        assert_case_equals(c.solve(prob), want_solve, "plain solve afterwards")  # (a new upload ...)
        for s in ("variants", "cases"):
            with pytest.raises(MagnetiteError) as e:  # ... drops them too
                c.download_sensitivity(s, 0)
            assert e.value.code == MAG_ERR_STATE
        c.sensitivities("run")
        c.run()
        with pytest.raises(MagnetiteError) as e:
            c.download_sensitivity("run", 0)
        assert e.value.code == MAG_ERR_STATE
