"""CPU: the neo-Hooke twin of tests/hyper_ref.py alone -- its stress and tangent by central differences, its linearisation, a rigid
motion, the local solve of the plane-stress condition, a homogeneous strip against a scalar root-find, the beam, and the SVK leg
of the restated loops against the three existing twins, bit for bit.

Bars.  Central differences with h = 1e-6 leave h^2 times a third derivative (1e-12 relative) and eps / h (2e-10) of round-off:
1e-9 of the largest entry.  K_T(0) against the linear tangent, and everything "at round-off": 16 eps = 3.6e-15 (the rotation: 4 eps |u| / edge, the round-off of H).  The strip
against the closed form: the run goes two iterations past convergence, on to its round-off floor, so 1e-13 (round-off times the
condition of K_T,FF, 6e2).
Measured: S 3e-11, K_T 2e-10 (triangle), 5e-11 (plate16); K_T(0) 3.0e-16; the rotation 7e-17 of mu |g| V; the local solve at most
11 iterations, d within 2 ulp of the root; the strip 3e-15."""
import numpy as np
import pytest
import scipy.optimize

import explicit_tl_cases as tlc
import hyper_ref as hr
import newton_ref as nr
import transient_tl_cases as ttc
from magnetite_amd import meshgen

EPS = np.finfo(np.float64).eps
NH = "neo_hooke"


def one_triangle():
    rng = np.random.default_rng(11)
    xy = np.array([[0.0, 0.0], [1.0, 0.1], [0.2, 0.9]]) + 0.05 * rng.uniform(-1, 1, (3, 2))
    return xy, np.array([[0, 1, 2]]), 69e9, 0.33, 0.5


def test_the_stress_is_twice_the_derivative_of_the_energy():
    xy, conn, E, nu, t = one_triangle()
    rng = np.random.default_rng(12)
    A = rng.uniform(-0.2, 0.2, (2, 2))
    C0 = (np.eye(2) + A).T @ (np.eye(2) + A)

    def W_of(C):  # the energy density at the symmetric stretch U = sqrt(C), which has this C
        w, Q = np.linalg.eigh(C)
        H = (Q * np.sqrt(w)) @ Q.T - np.eye(2)
        st = hr.neo_state(xy, conn, E, nu, t, ((xy - xy[0]) @ H.T).reshape(-1))
        return float(st["W"][0] / st["V"][0]), st

    _, st = W_of(C0)
    S = np.array([st["S"][0][0], st["S"][1][0], st["S"][2][0]])
    h = 1e-6
    dirs = (np.array([[1.0, 0], [0, 0]]), np.array([[0, 0], [0, 1.0]]), np.array([[0, 1.0], [1.0, 0]]))
    fd = np.array([(W_of(C0 + h * D)[0] - W_of(C0 - h * D)[0]) / (2 * h) for D in dirs]) * np.array([2.0, 2.0, 1.0])
    err = np.abs(fd - S).max() / np.abs(S).max()
    print("S against 2 dW/dC", err)
    assert err <= 1e-9


@pytest.mark.parametrize("which", ["triangle", "plate16"])
def test_the_tangent_is_the_derivative_of_the_force(which):
    if which == "triangle":
        xy, conn, E, nu, t = one_triangle()
        u = np.random.default_rng(13).uniform(-0.15, 0.15, 6)
    else:
        p = nr.case_problem("plate16", "load300")
        xy, conn, E, nu, t = hr.of_problem(p)
        u = hr.finite_state(p, 0.2)
    K = hr.tangent(NH, xy, conn, E, nu, t, u).toarray()
    h = 1e-6 * np.ptp(np.asarray(xy)[:, 0])
    fd = np.empty_like(K)
    for j in range(u.size):
        e = np.zeros(u.size)
        e[j] = h
        fd[:, j] = (hr.force(NH, xy, conn, E, nu, t, u + e)[0] - hr.force(NH, xy, conn, E, nu, t, u - e)[0]) / (2 * h)
    err = np.abs(fd - K).max() / np.abs(K).max()
    sym = np.abs(K - K.T).max() / np.abs(K).max()
    print(which, "K_T against the central difference of f_int", err, "asymmetry", sym, "min det F", hr.force(NH, xy, conn, E, nu, t, u)[2])
    assert err <= 1e-9 and sym <= 16 * EPS


def test_the_linearisation_is_k():
    p = nr.case_problem("beam", "beam")
    a = hr.of_problem(p)
    zero = np.zeros(2 * p.mesh.num_nodes)
    K0, Ks = hr.tangent(NH, *a, zero), nr.tangent(*a, zero)
    err = abs(K0 - Ks).max() / abs(Ks).max()
    print("K_T(0) against the St. Venant-Kirchhoff twin's", err)
    assert err <= 16 * EPS


def test_a_rigid_motion_and_the_reference_state():
    p = nr.case_problem("plate16", "load300")
    a = hr.of_problem(p)
    f, W, det = hr.force(NH, *a, tlc.rigid_motion(p))
    st = hr.neo_state(*a, np.zeros(2 * p.mesh.num_nodes))
    scale = float(st["mu"] * (np.abs(hr.shape_gradients(*a[:2])).max(axis=(1, 2)) * st["V"]).max())  # mu |g| V
    # (H is a difference of displacements over an edge: its round-off is eps |u| / edge, here eps times `lever`)
    u_rot = tlc.rigid_motion(p)
    lever = np.abs(u_rot).max() / np.sqrt(np.abs(st["twoA"]).min())
    print("rotation by 90 degrees plus a shift: |f| / (mu |g| V)", np.abs(f).max() / scale, "in eps * lever", np.abs(f).max() / scale / (EPS * lever),
          "W / (mu V)", W / float(st["mu"] * st["V"].sum()))
    assert np.abs(f).max() <= 4 * EPS * lever * scale and abs(det - 1.0) <= 4 * EPS * lever
    f0, W0, det0 = hr.force(NH, *a, np.zeros(2 * p.mesh.num_nodes))
    assert not f0.any() and W0 == 0.0 and det0 == 1.0
    assert not hr.neo_element_rows(*a, np.zeros(2 * p.mesh.num_nodes))[:, [0, 1, 2, 3, 4, 5, 7]].any()


def test_the_local_solve():
    j2m1 = np.concatenate([np.logspace(-6, 6, 481) - 1.0, [0.0], np.linspace(-1e-8, 1e-8, 21)])
    LD = np.longdouble
    worst_its, worst_g = 0, 0.0
    for nu in (0.0, 0.1, 0.3, 0.45, 0.49, 0.499):
        mu, lam = hr.lame(1.0, nu)
        d, its = hr.thickness(j2m1, lam / mu, counts=True)
        # the distance to the root in ulp of d: the Newton correction |g / g'| from the residual in np.longdouble
        half = LD(lam / mu) / 2
        step = np.abs(LD(d) + half * (np.log1p(LD(j2m1)) + np.log1p(LD(d)))) / (1 + half / (1 + LD(d)))
        g = step / np.maximum(np.abs(LD(d)), LD(1e-300))
        print("nu", nu, "iterations at most", its.max(), "distance of d from the root, in ulp of d", float(g.max() / EPS))
        worst_its, worst_g = max(worst_its, its.max()), max(worst_g, float(g.max()))
        assert np.isfinite(d).all() and (d > -1.0).all()
        if nu == 0.0:
            assert not d.any()
    assert worst_its <= 15 < hr.SOLVE_CAP and worst_g <= 8 * EPS
    # nu < 0: the iterate falls to the root after its first step (moderate states: far in compression no root exists)
    mu, lam = hr.lame(1.0, -0.3)
    m = np.linspace(-0.5, 1.0, 31)
    d, its = hr.thickness(m, lam / mu, counts=True)
    half = LD(lam / mu) / 2
    g = np.abs(LD(d) + half * (np.log1p(LD(m)) + np.log1p(LD(d)))) / (1 + half / (1 + LD(d))) / np.maximum(np.abs(LD(d)), LD(1e-300))
    print("nu -0.3: iterations at most", its.max(), "distance of d from the root, in ulp of d", float(g.max() / EPS))
    assert its.max() <= 15 and float(g.max()) <= 8 * EPS
    assert np.isnan(hr.thickness(np.array([np.nan]), 1.0)).all()


def uniaxial(stretch, E, nu):
    """(lateral stretch, S11) of the homogeneous uniaxial state: S22 = 0 gives C33 = l2^2, and S33 = 0 then
    mu (l2^2 - 1) + Lambda ln(l1 l2^2) = 0, a scalar equation for l2"""
    mu, lam = E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))
    l2 = scipy.optimize.brentq(lambda x: mu * (x * x - 1.0) + lam * np.log(stretch * x * x), 0.1, 10.0, xtol=1e-16, rtol=4 * EPS)
    return l2, mu * (1.0 - l2 * l2 / stretch ** 2)


@pytest.mark.parametrize("stretch, increments", [(0.5, 4), (1.5, 4)])
def test_the_strip_against_the_closed_form(stretch, increments):
    p = hr.strip_problem(stretch)
    xy, conn, E, nu, t = hr.of_problem(p)
    out = hr.newton(NH, xy, conn, E, nu, t, p.u_known, p.u_in, p.f_in, increments=increments, extra=2)
    l2, S11 = uniaxial(stretch, E, nu)
    x, y = p.mesh.xy[:, 0], p.mesh.xy[:, 1]
    right, top = x > x.max() - 1e-9, y > y.max() - 1e-9
    reaction = out["f"].reshape(-1, 2)[right, 0].sum()
    want = stretch * S11 * np.ptp(y) * t  # P11 = l1 S11 over the reference section
    lateral = out["u"].reshape(-1, 2)[top, 1] / np.ptp(y) + 1.0
    err_r, err_l = abs(reaction - want) / abs(want), np.abs(lateral - l2).max() / l2
    print("stretch", stretch, "iterations", out["newton_iterations"], "lateral stretch", l2, "reaction", want, "errors", err_r, err_l,
          "min det F", out["min_det"])
    assert out["converged"] and not out["inverted"]
    assert err_r <= 1e-13 and err_l <= 1e-13
    if stretch == 0.5:
        assert abs(l2 - 1.23515) < 5e-6 and list(out["newton_iterations"]) == [0, 4, 4, 4, 4] and abs(out["min_det"] - 0.61) < 0.01
        # St. Venant-Kirchhoff cannot compute this state: its tangent at the homogeneous state is indefinite
        free = np.flatnonzero(np.asarray(p.u_known) == 0)
        u_svk = np.stack([(stretch - 1.0) * x, (uniaxial_svk(stretch, nu) - 1.0) * y], axis=1).reshape(-1)
        w = np.linalg.eigvalsh(nr.tangent(xy, conn, E, nu, t, u_svk)[free][:, free].toarray())
        wn = np.linalg.eigvalsh(hr.tangent(NH, xy, conn, E, nu, t, out["u"])[free][:, free].toarray())
        print("negative eigenvalues of K_T,FF: St. Venant-Kirchhoff", int((w < 0).sum()), "neo-Hooke", int((wn < 0).sum()), "smallest / largest",
              wn[0] / wn[-1])
        assert (w < 0).sum() > 0 and wn[0] > 0


def uniaxial_svk(stretch, nu):
    """the lateral stretch of St. Venant-Kirchhoff's homogeneous uniaxial state: Eyy = -nu Exx"""
    return np.sqrt(1.0 - nu * (stretch ** 2 - 1.0))


def test_the_beam():
    p = nr.case_problem("beam", "beam")
    out, svk = hr.case_run(NH, "beam", "beam", 8), nr.case_run("beam", "beam", 8)
    tip = np.flatnonzero(p.mesh.xy[:, 0] > p.mesh.xy[:, 0].max() - 1e-9)
    d_nh, d_svk = out["u"].reshape(-1, 2)[tip].mean(axis=0), svk["u"].reshape(-1, 2)[tip].mean(axis=0)
    apart = np.linalg.norm(d_nh - d_svk) / np.linalg.norm(d_svk)
    print("beam, 8 increments: iterations", out["newton_iterations"], "min det F", out["min_det"], "tip", d_nh, "from St. Venant-Kirchhoff's", apart)
    assert list(out["newton_iterations"]) == [0] + [4] * 8 and abs(out["min_det"] - 0.96) < 0.005
    assert 1e-3 < apart < 1e-2  # (the laws differ visibly but mildly where strains are small)
    one = hr.case_run(NH, "beam", "beam", 1, 8)
    print("beam, 1 increment, line_search = 8: iterations", one["newton_iterations"], "halvings", one["halvings"])
    assert list(one["newton_iterations"]) == [0, 10] and one["halvings"] == 2
    assert np.linalg.norm(one["u"] - out["u"]) <= 1e-8 * np.linalg.norm(out["u"])


def same(a, b, keys):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_the_svk_leg_of_the_restated_loops_is_the_existing_twins():
    p = nr.case_problem("plate16", "load300")
    a = hr.of_problem(p)
    same(hr.newton("svk", *a, p.u_known, p.u_in, p.f_in, increments=2), nr.case_run("plate16", "load300", 2),
         ("u", "f", "newton_iterations", "residuals", "step_lengths", "states", "energies", "load", "min_det"))
    same(hr.newton("svk", *hr.of_problem(nr.case_problem("beam", "beam")), *(lambda q: (q.u_known, q.u_in, q.f_in))(nr.case_problem("beam", "beam")),
                   increments=1, line_search=2, load_factors=[1.1]), nr.path_run("energy2"),
         ("u", "f", "newton_iterations", "residuals", "step_lengths", "energies", "halvings"))
    s = tlc.setup("plate16", "load300")
    dt = tlc.dt_of("plate16", "load300")
    same(hr.explicit_tl("svk", *a, s["M"], s["free"], p.u_in, p.f_in, s["steps"], dt, s["alpha"], u0=s["u0"]), tlc.twin("plate16", "load300", dt),
         ("u", "v", "a", "f", "energies", "min_det"))
    s = ttc.setup("plate16", "load300")
    same(hr.newmark_tl("svk", *a, s["M"], s["free"], p.u_in, p.f_in, s["steps"], s["dt"], alpha=s["alpha"], u0=s["u0"], newton_tol=ttc.NEWTON_TOL),
         ttc.twin("plate16", "load300"), ("u", "v", "a", "f", "energies", "newton_iterations", "residuals", "min_det"))
    floor = hr.newmark_tl("svk", *a, s["M"], s["free"], p.u_in, p.f_in, s["steps"], s["dt"], alpha=s["alpha"], u0=s["u0"], newton_tol=ttc.NEWTON_TOL,
                          extra=3)
    same(floor, ttc.twin("plate16", "load300", extra=3), ("u", "newton_iterations", "residuals"))


def test_the_laws_differ_and_the_per_law_functions_dispatch():
    p = nr.case_problem("plate16", "load300")
    a = hr.of_problem(p)
    u = hr.finite_state(p, 0.1)
    f_s, f_n = hr.force("svk", *a, u)[0], hr.force(NH, *a, u)[0]
    assert np.array_equal(f_s, tlc.force_of(p, u)[0]) and np.abs(f_s - f_n).max() > 1e-3 * np.abs(f_s).max()
    assert np.array_equal(hr.element_rows("svk", *a, u), nr.element_rows(*a, u))
    assert np.array_equal(hr.element_rows(NH, *a, u)[:, [0, 1, 2, 6]], nr.element_rows(*a, u)[:, [0, 1, 2, 6]])
    sp = hr.spread(*a, u)
    print("the twin's own round-off against np.longdouble", sp)
    assert sp["force"] < 1e-13 and sp["tangent"] < 1e-14 and sp["rows"] < 1e-13
