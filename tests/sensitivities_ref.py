"""Reference for the sensitivity tests: a vectorised numpy restatement of 1/2 u_e^T K_e(x, nu) u_e -- K_e = (B^T D) B A t with the
signed area, as tests/numpy_twin.py states solver.rs:263-278 -- that accepts complex coordinates and a complex nu, so that the
derivatives come from the complex step (exact to round-off, no step-size error); and the potential energy of a problem solved
by the twin's direct solve, for the finite-difference checks.  The node gradient is evaluated in numpy's extended precision
(complex long double) and rounded once at the end, so its round-off is that of the result, not of the corner terms that
largely cancel in it; `dxy_ext` keeps the unrounded entries."""
import math
import dataclasses

import numpy as np

import numpy_twin

SCALARS = ("strain_energy", "potential_energy", "external_work", "reaction_work", "dPi_dE", "dPi_dnu", "dPi_dt")
STEP = 1e-30  # complex step: the imaginary part carries the derivative, nothing cancels


def element_stiffness(xy, conn, nu, youngs, t):
    """(E, 6, 6): K_e of every element; xy (N, 2) and nu may be complex."""
    p = np.asarray(xy)[conn]
    x, y = p[..., 0], p[..., 1]
    area = 0.5 * (x[:, 0] * (y[:, 1] - y[:, 2]) + x[:, 1] * (y[:, 2] - y[:, 0]) + x[:, 2] * (y[:, 0] - y[:, 1]))
    b = np.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], axis=1)
    g = np.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], axis=1)
    B = np.zeros((len(conn), 3, 6), dtype=np.result_type(p.dtype, np.float64))
    B[:, 0, 0::2] = b
    B[:, 1, 1::2] = g
    B[:, 2, 0::2] = g
    B[:, 2, 1::2] = b
    B = B / (2.0 * area)[:, None, None]
    D = np.array([[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]]) * (youngs / (1 - nu ** 2))
    return np.einsum("eki,kl,elj->eij", B, D, B) * (area * t)[:, None, None]


def element_energy(xy, conn, u, nu, youngs, t):
    """(E,): 1/2 u_e^T K_e u_e."""
    ue = np.asarray(u).reshape(-1, 2)[conn].reshape(len(conn), 6)
    return 0.5 * np.einsum("ei,eij,ej->e", ue, element_stiffness(xy, conn, nu, youngs, t), ue)


def sensitivities(xy, conn, u_known, u, f_out, u_in, f_in, youngs, nu, t):
    """What mag_run_sensitivities computes for one solved member: dict(energy, dxy, and SCALARS by name)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    conn = np.asarray(conn).reshape(-1, 3)
    energy = element_energy(xy, conn, u, nu, youngs, t)
    dxy = np.zeros(xy.size, dtype=np.longdouble)
    ext_nu, ext_e, ext_t = np.longdouble(nu), np.longdouble(youngs), np.longdouble(t)
    for corner in range(3):
        for d in range(2):  # every element's own copy of its corner moves: the derivative of ITS energy, then gathered
            z = xy.astype(np.clongdouble)[conn]
            z[:, corner, d] += 1j * STEP
            pts = z.reshape(-1, 2)  # a mesh of disjoint triangles
            own = np.arange(3 * len(conn)).reshape(-1, 3)
            ue = np.asarray(u, dtype=np.longdouble).reshape(-1, 2)[conn].reshape(-1)
            de = element_energy(pts, own, ue, ext_nu, ext_e, ext_t).imag / STEP
            np.add.at(dxy, 2 * conn[:, corner] + d, de)
    dnu = float(np.sum(element_energy(xy, conn, u, nu + 1j * STEP, youngs, t).imag) / STEP)
    W = float(np.sum(energy))
    free = np.asarray(u_known) == 0
    ext = float(np.sum(np.asarray(f_in)[free] * np.asarray(u)[free]))
    react = float(np.sum(np.asarray(f_out)[~free] * np.asarray(u_in)[~free]))
    return dict(energy=energy, dxy=dxy.astype(np.float64), dxy_ext=dxy, strain_energy=W, potential_energy=W - ext, external_work=ext, reaction_work=react,
                dPi_dE=W / youngs, dPi_dnu=dnu, dPi_dt=W / t)


def of_solution(prob, sol, xy=None, material=None, u_in=None, f_in=None):
    """sensitivities() of problem `prob` (or of its variant xy / material / values) for a solution dict with u and f."""
    mat = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness) if material is None else material
    return sensitivities(prob.mesh.xy if xy is None else xy, prob.mesh.conn, prob.u_known, sol["u"], sol["f"],
                         prob.u_in if u_in is None else u_in, prob.f_in if f_in is None else f_in, mat[0], mat[1], mat[2])


def direct_solution(prob):
    """u, f of the twin's direct solve."""
    s = numpy_twin.solve(prob.mesh.xy, prob.mesh.conn, prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus,
                         prob.poisson_ratio, prob.part_thickness)
    return dict(u=s["u"], f=s["f"])


def potential(prob):
    """Pi = W - f_F^T u_F at the direct solution of prob, W the sum of the element energies: both sums exact (fsum), so that a
    difference quotient of Pi carries the round-off of the terms only (u^T (K u) cancels row by row and is noisier)."""
    s = numpy_twin.solve(prob.mesh.xy, prob.mesh.conn, prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus,
                         prob.poisson_ratio, prob.part_thickness)
    free = prob.u_known == 0
    energy = element_energy(np.asarray(prob.mesh.xy, dtype=np.float64).reshape(-1, 2), np.asarray(prob.mesh.conn).reshape(-1, 3),
                            s["u"], prob.poisson_ratio, prob.youngs_modulus, prob.part_thickness)
    return math.fsum(energy) - math.fsum(prob.f_in[free] * s["u"][free])


def moved(prob, dof, step):
    """prob with coordinate `dof` (2 * node + axis) moved by step."""
    xy = prob.mesh.xy.copy().reshape(-1)
    xy[dof] += step
    return dataclasses.replace(prob, mesh=dataclasses.replace(prob.mesh, xy=xy.reshape(-1, 2)))
