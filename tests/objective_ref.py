"""Reference for the objective tests: the numpy statement of what mag_run_objective returns for one solved member -- J, g = dJ/du,
the explicit partials at fixed u (pxy, pJ_pE, pJ_pnu, pJ_pt) and, with the adjoint of adjoint_ref, the totals -- for the two
objectives of include/magnetite_hip.h.  sigma_e = D B u_e is written with the twin's D and B (numpy_twin.stress_strain,
strain_displacement: solver.rs:240-250, 204-230, the SIGNED area); derivatives come from the complex step (STEP, exact to
round-off) element by element, and the node sums run in numpy's extended precision and are rounded once, as sensitivities_ref
and adjoint_ref do.  `ext=False` evaluates the same expressions in float64 throughout: the gap between the two is the round-off
of the formula itself, which the GPU tests may allow for (OB)."""
import numpy as np

import adjoint_ref as aref
import sensitivities_ref as sref

STEP = sref.STEP
KINDS = ("disp_lsq", "stress_pnorm")
EXPLICIT = ("pJ_pE", "pJ_pnu", "pJ_pt")
TOTALS = ("dJ_dE", "dJ_dnu", "dJ_dt")


def element_stress(xy, conn, u, nu, youngs):
    """(E, 3): (sx, sy, txy) = D B u_e of every element; xy (N, 2), u, nu and youngs may be complex or extended."""
    p = np.asarray(xy)[conn]
    x, y = p[..., 0], p[..., 1]
    area = 0.5 * (x[:, 0] * (y[:, 1] - y[:, 2]) + x[:, 1] * (y[:, 2] - y[:, 0]) + x[:, 2] * (y[:, 0] - y[:, 1]))
    b = np.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], axis=1)
    g = np.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], axis=1)
    ue = np.asarray(u).reshape(-1, 2)[conn]
    ux, uy = ue[..., 0], ue[..., 1]
    d = 2.0 * area
    ex, ey, gxy = np.sum(b * ux, axis=1) / d, np.sum(g * uy, axis=1) / d, np.sum(g * ux + b * uy, axis=1) / d
    c = youngs / (1 - nu ** 2)
    return np.stack([c * (ex + nu * ey), c * (nu * ex + ey), c * ((1 - nu) / 2) * gxy], axis=1)


def von_mises_sq(sig):
    sx, sy, txy = sig[:, 0], sig[:, 1], sig[:, 2]
    return sx * sx - sx * sy + sy * sy + 3 * txy * txy


def pnorm_terms(xy, conn, u, nu, youngs, w, p, scale):
    """(E,): w_e (vm_e / scale)^p, as (vm_e^2 / scale^2)^(p/2) so that complex arguments pass; 0 where vm_e = 0."""
    t = von_mises_sq(element_stress(xy, conn, u, nu, youngs)) / (scale * scale)
    live = t.real > 0
    out = np.zeros(t.shape, dtype=t.dtype)
    out[live] = t[live] ** (p / 2)
    return out * w


def _types(ext):
    return (np.longdouble, np.clongdouble) if ext else (np.float64, np.complex128)


def stress_pnorm(xy, conn, u, youngs, nu, t, weights=None, p=8.0, scale=1.0, ext=True):
    """dict(J, S, g, pxy, pJ_pE, pJ_pnu, pJ_pt) of J = scale S^(1/p), S = sum_e w_e (vm_e / scale)^p; pJ_pnu_abs: the sum of the
    magnitudes of pJ_pnu's element terms, which may cancel in it."""
    real, cplx = _types(ext)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    conn = np.asarray(conn).reshape(-1, 3)
    u = np.asarray(u, dtype=np.float64)
    E = len(conn)
    w = (np.ones(E) if weights is None else np.asarray(weights, dtype=np.float64)).astype(real)
    r_nu, r_e, r_p, r_scale = real(nu), real(youngs), real(p), real(scale)
    S = np.sum(pnorm_terms(xy.astype(real), conn, u.astype(real), r_nu, r_e, w, r_p, r_scale))
    zeros = dict(J=0.0, S=0.0, g=np.zeros(u.size), pxy=np.zeros(u.size), pJ_pE=0.0, pJ_pnu=0.0, pJ_pt=0.0, pJ_pnu_abs=0.0)
    if not S > 0:
        return zeros
    J = r_scale * S ** (1 / r_p)
    dJ_dS = J / (r_p * S)
    own = np.arange(3 * E).reshape(-1, 3)  # a mesh of disjoint triangles: every element's own copy of its corner moves
    g, pxy = np.zeros(u.size, dtype=real), np.zeros(u.size, dtype=real)
    for corner in range(3):
        for d in range(2):
            z = xy.astype(cplx)[conn]
            ue = u.astype(cplx).reshape(-1, 2)[conn]
            z[:, corner, d] += 1j * STEP
            de = pnorm_terms(z.reshape(-1, 2), own, ue.reshape(-1), r_nu, r_e, w, r_p, r_scale).imag / STEP
            np.add.at(pxy, 2 * conn[:, corner] + d, de)
            z = xy.astype(cplx)[conn]
            ue[:, corner, d] += 1j * STEP
            de = pnorm_terms(z.reshape(-1, 2), own, ue.reshape(-1), r_nu, r_e, w, r_p, r_scale).imag / STEP
            np.add.at(g, 2 * conn[:, corner] + d, de)
    cu, cxy = u.astype(cplx), xy.astype(cplx)
    dnu_e = pnorm_terms(cxy, conn, cu, cplx(nu + 1j * STEP), r_e, w, r_p, r_scale).imag / STEP
    dnu = np.sum(dnu_e)
    dE = np.sum(pnorm_terms(cxy, conn, cu, r_nu, cplx(youngs * (1 + 1j * STEP)), w, r_p, r_scale).imag) / (STEP * r_e)
    return dict(J=float(J), S=float(S), g=(dJ_dS * g).astype(np.float64), pxy=(dJ_dS * pxy).astype(np.float64),
                pJ_pE=float(dJ_dS * dE), pJ_pnu=float(dJ_dS * dnu), pJ_pt=0.0, pJ_pnu_abs=float(dJ_dS * np.sum(np.abs(dnu_e))))


def disp_lsq(u, weights, target=None, ext=True):
    """dict(J, g, pxy, pJ_pE, pJ_pnu, pJ_pt) of J = sum_i w_i (u_i - target_i)^2: no explicit dependence on the design."""
    real, cplx = _types(ext)
    u = np.asarray(u, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64).astype(real)
    tg = (np.zeros(u.size) if target is None else np.asarray(target, dtype=np.float64)).astype(real)
    J = np.sum(w * (u.astype(real) - tg) ** 2)
    g = (w * ((u.astype(cplx) + 1j * STEP) - tg) ** 2).imag / STEP
    return dict(J=float(J), g=g.astype(np.float64), pxy=np.zeros(u.size), pJ_pE=0.0, pJ_pnu=0.0, pJ_pt=0.0, pJ_pnu_abs=0.0)


def objective(kind, xy, conn, u, youngs, nu, t, weights=None, target=None, p=8.0, scale=1.0, ext=True):
    if kind == "disp_lsq":
        return disp_lsq(u, weights, target, ext)
    assert kind == "stress_pnorm", kind
    return stress_pnorm(xy, conn, u, youngs, nu, t, weights, p, scale, ext)


def of_problem(kind, prob, u, xy=None, material=None, **spec):
    """objective() of problem `prob` (or of its variant xy / material) at displacements u."""
    mat = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness) if material is None else material
    return objective(kind, prob.mesh.xy if xy is None else xy, prob.mesh.conn, u, mat[0], mat[1], mat[2], **spec)


def with_totals(kind, prob, u, xy=None, material=None, **spec):
    """of_problem() plus the totals: explicit + adjoint (adjoint_ref.of_problem on g), dxy and dJ_dE, dJ_dnu, dJ_dt."""
    out = of_problem(kind, prob, u, xy, material, **spec)
    adj = aref.of_problem(prob, u, out["g"], xy, material)
    out["dxy"] = out["pxy"] + adj["dxy"]
    for total, part in zip(TOTALS, EXPLICIT):
        out[total] = out[part] + adj[total]
    out["adjoint"] = adj
    return out
