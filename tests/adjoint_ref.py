"""Reference for the adjoint tests: the numpy statement of what mag_run_adjoint returns for one solved member -- lambda, dloads,
delem, dxy and the scalars of include/magnetite_hip.h -- built on sensitivities_ref.element_stiffness (K_e = (B^T D) B A t with the
signed area), with complex coordinates and a complex nu for the derivatives and numpy's extended precision for the node sums, as
sensitivities_ref.sensitivities does; the adjoint solution itself from the twin's direct solve; and the two objectives the tests
differentiate."""
import numpy as np

import numpy_twin
import sensitivities_ref as ref

STEP = ref.STEP
SCALARS = ("a", "dJ_dE", "dJ_dnu", "dJ_dt")
DENSE_DOFS = 2000  # up to here the twin's dense solve (and its element loop) takes about a second


def bilinear(xy, conn, lam, u, nu, youngs, t):
    """(E,): lambda_e^T K_e u_e; xy, nu, lam and u may be complex or extended."""
    conn = np.asarray(conn).reshape(-1, 3)
    le = np.asarray(lam).reshape(-1, 2)[conn].reshape(len(conn), 6)
    ue = np.asarray(u).reshape(-1, 2)[conn].reshape(len(conn), 6)
    return np.einsum("ei,eij,ej->e", le, ref.element_stiffness(xy, conn, nu, youngs, t), ue)


def adjoint(xy, conn, u_known, u, lam, g, f_adj, youngs, nu, t):
    """What mag_run_adjoint computes for one member with displacements u, adjoint solution lam (K_ff lam_F = g_F, 0 on the
    prescribed DOFs) and adjoint forces f_adj ((K lam) on the prescribed DOFs): dict(lambda, dloads, delem, dxy, and SCALARS)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    conn = np.asarray(conn).reshape(-1, 3)
    u, lam, g, f_adj = (np.asarray(v, dtype=np.float64) for v in (u, lam, g, f_adj))
    bil = bilinear(xy, conn, lam, u, nu, youngs, t)
    dxy = np.zeros(xy.size, dtype=np.longdouble)
    ext_nu, ext_e, ext_t = np.longdouble(nu), np.longdouble(youngs), np.longdouble(t)
    own = np.arange(3 * len(conn)).reshape(-1, 3)  # a mesh of disjoint triangles: every element's own copy of its corner moves
    ue = u.astype(np.longdouble).reshape(-1, 2)[conn].reshape(-1)
    le = lam.astype(np.longdouble).reshape(-1, 2)[conn].reshape(-1)
    for corner in range(3):
        for d in range(2):
            z = xy.astype(np.clongdouble)[conn]
            z[:, corner, d] += 1j * STEP
            de = bilinear(z.reshape(-1, 2), own, le, ue, ext_nu, ext_e, ext_t).imag / STEP
            np.add.at(dxy, 2 * conn[:, corner] + d, -de)
    dnu = -float(np.sum(bilinear(xy, conn, lam, u, nu + 1j * STEP, youngs, t).imag) / STEP)
    a = float(np.sum(bil))
    known = np.asarray(u_known) == 1
    out = {"lambda": lam, "dloads": np.where(known, g - f_adj, lam), "delem": -bil, "dxy": dxy.astype(np.float64)}
    out.update(a=a, dJ_dE=-a / youngs, dJ_dnu=dnu, dJ_dt=-a / t)
    return out


def direct_adjoint(xy, conn, u_known, g, youngs, nu, t):
    """lambda and the adjoint forces of K_ff lambda_F = g_F: numpy_twin.solve with u_in = 0, f_in = g.  Past DENSE_DOFS unknowns
    the same system -- the same K_e, summed in a sparse matrix -- goes through a sparse LU with one step of refinement instead of
    the twin's dense solve and per-element Python loop, which take many seconds per mesh there (the two agree to 1e-13)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    conn = np.asarray(conn).reshape(-1, 3)
    g = np.asarray(g, dtype=np.float64)
    if g.size <= DENSE_DOFS:
        s = numpy_twin.solve(xy, conn, np.asarray(u_known), np.zeros(g.size), g, youngs, nu, t)
        return s["u"], s["f"]
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    dofs = np.stack([2 * conn, 2 * conn + 1], axis=2).reshape(len(conn), 6)
    K = sp.csr_matrix((ref.element_stiffness(xy, conn, nu, youngs, t).reshape(-1),
                       (np.repeat(dofs, 6, axis=1).reshape(-1), np.tile(dofs, (1, 6)).reshape(-1))), shape=(g.size, g.size))
    free = np.where(np.asarray(u_known) == 0)[0]
    Kff = K[free][:, free].tocsc()
    lu = splu(Kff)
    x = lu.solve(g[free])
    x += lu.solve(g[free] - Kff @ x)
    lam = np.zeros(g.size)
    lam[free] = x
    f = g.copy()
    known = np.asarray(u_known) == 1
    f[known] = (K @ lam)[known]
    return lam, f


def of_problem(prob, u, g, xy=None, material=None):
    """adjoint() of problem `prob` (or of its variant xy / material) at displacements u for dJ/du = g, lambda from direct_adjoint."""
    mat = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness) if material is None else material
    xy = prob.mesh.xy if xy is None else xy
    lam, f_adj = direct_adjoint(xy, prob.mesh.conn, prob.u_known, g, mat[0], mat[1], mat[2])
    return adjoint(xy, prob.mesh.conn, prob.u_known, u, lam, g, f_adj, mat[0], mat[1], mat[2])


# ---- the objectives
def patch_weights(prob, radius=0.3, seed=7):
    """(2N,) w >= 0, supported on the DOFs of the nodes within `radius` (of the part's extent) of its centre: J1 = sum w u^2."""
    xy = np.asarray(prob.mesh.xy).reshape(-1, 2)
    lo, span = xy.min(axis=0), np.ptp(xy, axis=0).max()
    inside = np.linalg.norm((xy - lo) / span - 0.5 * np.ptp(xy, axis=0) / span, axis=1) <= radius
    assert inside.sum() >= 4
    w = np.random.default_rng(seed).uniform(0.5, 1.5, xy.size)
    return np.where(np.repeat(inside, 2), w, 0.0)


def J1(w, u):
    return float(np.sum(w * u * u))


def dJ1(w, u):
    return 2.0 * w * u
