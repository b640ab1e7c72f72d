"""Reference for the stress recovery tests: the numpy statement of what mag_run_stress returns for one solved member
(include/magnetite_hip.h) -- the tensor sigma_e = D B u_e and its von Mises value per element, the |A|-weighted nodal average
(np.add.at: the sums run in element order, which is the order of a node's incidence list), the Zienkiewicz-Zhu indicator as
the exact triangle integral of (sigma* - sigma_e)^T C (sigma* - sigma_e) t, and the scalars."""
import numpy as np

import objective_ref as oref


def areas(xy, conn):
    """(E,): the SIGNED areas."""
    p = np.asarray(xy).reshape(-1, 2)[conn]
    x, y = p[..., 0], p[..., 1]
    return 0.5 * (x[:, 0] * (y[:, 1] - y[:, 2]) + x[:, 1] * (y[:, 2] - y[:, 0]) + x[:, 2] * (y[:, 0] - y[:, 1]))


def compliance(s, nu, youngs):
    """s^T C s of tensors s (..., 3), C = D^-1."""
    sx, sy, txy = s[..., 0], s[..., 1], s[..., 2]
    return (sx * sx - 2 * nu * sx * sy + sy * sy + 2 * (1 + nu) * txy * txy) / youngs


def von_mises(s):
    sx, sy, txy = s[..., 0], s[..., 1], s[..., 2]
    return np.sqrt(sx * sx - sx * sy + sy * sy + 3 * txy * txy)


def triangle_integral(corner_values, sigma_e, area, nu, youngs, t):
    """(E,): the integral over every triangle of (s - sigma_e)^T C (s - sigma_e) t, s interpolated linearly between
    corner_values (E, 3, 3): |A| t / 12 (sum_k d_k^T C d_k + (sum_k d_k)^T C (sum_k d_k)) -- exact for a linear s."""
    d = corner_values - sigma_e[:, None, :]
    return np.abs(area) * t / 12 * (compliance(d, nu, youngs).sum(axis=1) + compliance(d.sum(axis=1), nu, youngs))


def nodal_average(sig, area, conn, num_nodes):
    """(N, 3): the |A|-weighted average of the tensors of every node's triangles; zeros for a node that no element touches."""
    num, den = np.zeros((num_nodes, 3)), np.zeros(num_nodes)
    a = np.abs(area)
    idx = conn.reshape(-1)  # element after element: per node the order of its incidence list
    np.add.at(num, idx, np.repeat(a[:, None] * sig, 3, axis=0))
    np.add.at(den, idx, np.repeat(a, 3))
    out = np.zeros((num_nodes, 3))
    live = den > 0
    out[live] = num[live] / den[live, None]
    return out


def stress_recovery(xy, conn, u, youngs, nu, t):
    """dict(elem (E, 4), node (N, 4), eta2 (E), eta_sq, energy_sq, eta_rel, vm_max, vm_node_max) of one solved member."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    conn = np.asarray(conn).reshape(-1, 3)
    u = np.asarray(u, dtype=np.float64)
    sig = oref.element_stress(xy, conn, u, nu, youngs)
    area = areas(xy, conn)
    star = nodal_average(sig, area, conn, len(xy))
    eta2 = triangle_integral(star[conn], sig, area, nu, youngs, t)
    eta_sq = float(np.sum(eta2))
    energy_sq = float(np.sum(np.abs(area) * t * compliance(sig, nu, youngs)))
    total = energy_sq + eta_sq
    return dict(elem=np.column_stack([sig, von_mises(sig)]), node=np.column_stack([star, von_mises(star)]), eta2=eta2,
                eta_sq=eta_sq, energy_sq=energy_sq, eta_rel=float(np.sqrt(eta_sq / total)) if total > 0 else 0.0,
                vm_max=float(von_mises(sig).max()), vm_node_max=float(von_mises(star).max()))


def of_problem(prob, u, xy=None, material=None):
    """stress_recovery() of problem `prob` (or of its variant xy / material) at displacements u."""
    mat = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness) if material is None else material
    return stress_recovery(prob.mesh.xy if xy is None else xy, prob.mesh.conn, u, mat[0], mat[1], mat[2])


def cancellation(out):
    """|sigma| / |d| in the energy norm, sqrt(U^2 / eta^2): the factor by which the relative round-off of d = sigma* - sigma_e
    exceeds that of the tensors it is the difference of."""
    return float(np.sqrt(out["energy_sq"] / out["eta_sq"])) if out["eta_sq"] > 0 else float("inf")
