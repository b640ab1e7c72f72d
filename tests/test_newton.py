"""CPU: the numpy twin of the nonlinear-statics pass (tests/newton_ref.py) on its own -- the tangent against the project's K, its
symmetry, a central difference of the internal force, a rigid motion, and the convergence of the Newton loop on the cases the GPU
tests hold the device against.  Figures measured here: tangent(0) - K exactly 0; symmetry 0; the central difference 6e-12
(plate16), 1.3e-10 (beam); the beam in 8 increments 4 iterations each, smallest det F 0.9575; load300 in 2 increments 4-5 and 4;
pull5 in 1 increment 4 with the predictor, 6-12 when the supports jump first."""
import numpy as np
import pytest

import explicit_tl_cases as cases
import explicit_tl_ref as tl
import modal_ref
import newton_ref as nr

TOL = 1e-10


def test_the_tangent_at_zero_is_k_and_symmetric():
    for name, kind in (("beam", "beam"), ("plate16", "load300"), ("two_fans", "pull5")):
        p = nr.case_problem(name, kind)
        K = modal_ref.matrices(p, cases.RHO, True)[0]
        KT = nr.tangent(*nr.of_problem(p), np.zeros(2 * p.mesh.num_nodes))
        big = abs(K).max()
        print(name, "tangent(0) - K", abs(KT - K).max() / big, "asymmetry", abs(KT - KT.T).max() / big)
        assert abs(KT - K).max() <= 1e-14 * big
        assert abs(KT - KT.T).max() <= 1e-15 * big


@pytest.mark.parametrize("name, kind, increments", [("plate16", "load300", 2), ("beam", "beam", 8)])
def test_the_tangent_is_the_derivative_of_the_force(name, kind, increments):
    p = nr.case_problem(name, kind)
    a = nr.of_problem(p)
    u = nr.case_run(name, kind, increments)["u"]
    KT = nr.tangent(*a, u)
    assert abs(KT - KT.T).max() <= 1e-15 * abs(KT).max()
    L = np.ptp(p.mesh.xy[:, 0])
    rng = np.random.default_rng(5)
    for _ in range(3):
        d = rng.uniform(-1.0, 1.0, u.size)
        eps = 1e-6 * L
        fd = (tl.tl_force(*a, u + eps * d)[0] - tl.tl_force(*a, u - eps * d)[0]) / (2.0 * eps)
        err = np.linalg.norm(fd - KT @ d) / np.linalg.norm(KT @ d)
        print(name, "central difference against K_T d", err)
        assert err <= 1e-8


def test_an_infinitesimal_rotation_of_a_rotated_part_is_in_the_null_space():
    p = nr.case_problem("plate16", "load300")
    u = cases.rigid_motion(p)
    KT = nr.tangent(*nr.of_problem(p), u)
    x = p.mesh.xy + u.reshape(-1, 2)  # the rotated part; its centre is the centroid moved by (0.3, -0.2)
    c = x.mean(axis=0)
    w = np.stack([-(x[:, 1] - c[1]), x[:, 0] - c[0]], axis=1).reshape(-1)
    got = np.linalg.norm(KT @ w) / (abs(KT).max() * np.linalg.norm(w))
    print("|K_T w| / (|K_T| |w|) at the rigid motion", got)
    assert got <= 1e-10
    assert np.linalg.norm(nr.tangent(*nr.of_problem(p), 0 * u) @ w) > 1e-3 * abs(KT).max() * np.linalg.norm(w)  # (K alone is not blind to it)


def margins(out):
    """every increment's last-but-one ratio >= 100 tol or its last <= tol / 5: a device count that differs is a real finding"""
    at = 0
    for n in out["newton_iterations"][1:]:
        r = out["residuals"][at:at + n]
        assert r[-1] <= TOL
        assert (n == 1 or r[-2] >= 100 * TOL) or r[-1] <= TOL / 5, r
        at += n


def test_the_beam_converges_as_measured():
    p = nr.case_problem("beam", "beam")
    out = nr.case_run("beam", "beam", 8)
    tip = np.flatnonzero(p.mesh.xy[:, 0] > p.mesh.xy[:, 0].max() - 1e-9)
    print("beam: iterations", out["newton_iterations"], "tip u", out["u"].reshape(-1, 2)[tip], "min det F", out["min_det"])
    assert out["converged"] and out["halvings"] == 0
    assert all(abs(n - 4) <= 1 for n in out["newton_iterations"][1:])
    assert abs(out["min_det"] - 0.9575) <= 1e-3
    assert np.allclose(out["load"], np.arange(9) / 8)
    mid = out["u"].reshape(-1, 2)[tip].mean(axis=0)
    assert 0.25 <= -mid[1] <= 0.29 and mid[0] < -0.03  # (the tip comes down a quarter of the length and in by a few percent)
    margins(out)


@pytest.mark.parametrize("increments", [1, 4])
def test_the_line_search_reaches_the_same_equilibrium(increments):
    want = nr.case_run("beam", "beam", 8)["u"]
    out = nr.case_run("beam", "beam", increments, line_search=10)
    err = np.linalg.norm(out["u"] - want) / np.linalg.norm(want)
    print("beam,", increments, "increments with line search: iterations", out["newton_iterations"], "halvings", out["halvings"], "u apart", err)
    assert out["converged"] and out["halvings"] > 0 and err <= 1e-8


@pytest.mark.parametrize("name", cases.FOUR)
def test_load300_and_pull5_converge_as_measured(name):
    load = nr.case_run(name, "load300", 2)
    pull = nr.case_run(name, "pull5", 1)
    print(name, "load300", load["newton_iterations"], "pull5", pull["newton_iterations"])
    assert load["converged"] and pull["converged"]
    assert all(3 <= n <= 6 for n in load["newton_iterations"][1:])
    assert abs(pull["newton_iterations"][1] - 4) <= 1
    margins(load)
    margins(pull)


def test_the_predictor_saves_iterations():
    p = nr.case_problem("frontal3k", "pull5")
    jump = nr.newton(*nr.of_problem(p), p.u_known, p.u_in, p.f_in, increments=1, predictor=False)
    with_it = nr.case_run("frontal3k", "pull5", 1)
    print("frontal3k pull5: predictor", with_it["newton_iterations"][1], "jump", jump["newton_iterations"][1])
    assert jump["converged"] and jump["newton_iterations"][1] >= with_it["newton_iterations"][1] + 2
    assert np.linalg.norm(jump["u"] - with_it["u"]) <= 1e-8 * np.linalg.norm(with_it["u"])


def test_the_cap_leaves_the_start():
    out = nr.case_run("beam", "beam", 1, max_newton=2)
    assert not out["converged"] and out["converged_increments"] == 0 and not out["u"].any() and len(out["residuals"]) == 2
