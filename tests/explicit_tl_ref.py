"""Reference for the total-Lagrangian explicit-dynamics tests (CPU, numpy only; not product): the internal force of a
St. Venant-Kirchhoff plane-stress material in the reference configuration as include/magnetite_hip.h states it for
MAG_KIN_TOTAL_LAGRANGIAN, written from the formulas with np.add.at, and explicit_ref.explicit with K @ w replaced by it.

  triangle (a, b, c):  db = X_b - X_a, dc = X_c - X_a, ub = u_b - u_a, uc = u_c - u_a, 2A = db x dc
  H = grad u:   H11 = (dc.y ub.x - db.y uc.x) / 2A   H12 = (db.x uc.x - dc.x ub.x) / 2A
                H21 = (dc.y ub.y - db.y uc.y) / 2A   H22 = (db.x uc.y - dc.x ub.y) / 2A       F = I + H
  E = (F^T F - I) / 2,  S = c [[Exx + nu Eyy, h Gxy], [h Gxy, Eyy + nu Exx]],  c = E / (1 - nu^2),  h = (1 - nu) / 2,  P = F S
  the force on a corner is A t P grad N (on a: (t / 2) P (db.y - dc.y, dc.x - db.x)^T, the others by cyclic shift)
  W_e = A t (Sxx Exx + Syy Eyy + Sxy Gxy) / 2

  step       a' = (amp[n+1] f - alpha m vt - f_int(ut))_F / ((1 + dt alpha / 2) m)
  reactions  f_int(u) on P, amp[n] f on F
  energies   T = 1/2 v.mv,  W = sum_e W_e,  P = amp[n] f_F . u_F"""
import numpy as np


def strains(xy, conn, u):
    """per element: 2A, H (E, 2, 2), (Exx, Eyy, Gxy)"""
    xy = np.asarray(xy, dtype=np.float64)
    U = np.asarray(u, dtype=np.float64).reshape(-1, 2)
    a, b, c = conn[:, 0], conn[:, 1], conn[:, 2]
    db, dc = xy[b] - xy[a], xy[c] - xy[a]
    ub, uc = U[b] - U[a], U[c] - U[a]
    twoA = db[:, 0] * dc[:, 1] - dc[:, 0] * db[:, 1]
    H = np.empty((conn.shape[0], 2, 2))
    H[:, 0, 0] = (dc[:, 1] * ub[:, 0] - db[:, 1] * uc[:, 0]) / twoA
    H[:, 0, 1] = (db[:, 0] * uc[:, 0] - dc[:, 0] * ub[:, 0]) / twoA
    H[:, 1, 0] = (dc[:, 1] * ub[:, 1] - db[:, 1] * uc[:, 1]) / twoA
    H[:, 1, 1] = (db[:, 0] * uc[:, 1] - dc[:, 0] * ub[:, 1]) / twoA
    Exx = H[:, 0, 0] + 0.5 * (H[:, 0, 0] ** 2 + H[:, 1, 0] ** 2)
    Eyy = H[:, 1, 1] + 0.5 * (H[:, 0, 1] ** 2 + H[:, 1, 1] ** 2)
    Gxy = H[:, 0, 1] + H[:, 1, 0] + H[:, 0, 0] * H[:, 0, 1] + H[:, 1, 0] * H[:, 1, 1]
    return twoA, H, (Exx, Eyy, Gxy)


def tl_force(xy, conn, E, nu, t, u):
    """f_int(u) (2N), W(u), the smallest det F"""
    xy = np.asarray(xy, dtype=np.float64)
    conn = np.asarray(conn, dtype=np.int64)
    twoA, H, (Exx, Eyy, Gxy) = strains(xy, conn, u)
    c = E / (1.0 - nu * nu)
    Sxx, Syy, Sxy = c * (Exx + nu * Eyy), c * (Eyy + nu * Exx), c * (1.0 - nu) / 2.0 * Gxy
    F = H + np.eye(2)[None]
    S = np.empty_like(H)
    S[:, 0, 0], S[:, 1, 1], S[:, 0, 1], S[:, 1, 0] = Sxx, Syy, Sxy, Sxy
    P = F @ S
    f = np.zeros((xy.shape[0], 2))
    for k in range(3):  # corner k sees the triangle as (a, b, c) = (k, k + 1, k + 2)
        a, b, cc = conn[:, k], conn[:, (k + 1) % 3], conn[:, (k + 2) % 3]
        db, dc = xy[b] - xy[a], xy[cc] - xy[a]
        n = np.stack([db[:, 1] - dc[:, 1], dc[:, 0] - db[:, 0]], axis=1)
        np.add.at(f, a, (t / 2.0) * np.einsum("eij,ej->ei", P, n))
    W = float(np.sum(0.5 * twoA * t * (Sxx * Exx + Syy * Eyy + Sxy * Gxy) / 2.0))
    det = F[:, 0, 0] * F[:, 1, 1] - F[:, 0, 1] * F[:, 1, 0]
    return f.reshape(-1), W, float(det.min())


def explicit_tl(xy, conn, E, nu, t, M, free, u_in, f_in, steps, dt, alpha=0.0, amplitude=None, u0=None, v0=None):
    """explicit_ref.explicit with K @ (ut + eta vt) replaced by tl_force(ut) (eta = 0): dict(u, v, a, f (steps + 1, 2N each),
    energies (steps + 1, 3 = T, W, P), min_det (the smallest det F of any force evaluation))."""
    n = 2 * np.asarray(xy).shape[0]
    known = np.ones(n, dtype=bool)
    known[free] = False
    m = np.asarray(M.diagonal(), dtype=np.float64)
    amp = np.ones(steps + 1) if amplitude is None else np.asarray(amplitude, dtype=np.float64)
    f = np.where(known, 0.0, np.asarray(f_in, dtype=np.float64))
    u_in = np.asarray(u_in, dtype=np.float64)
    u = np.where(known, u_in, 0.0 if u0 is None else np.asarray(u0, dtype=np.float64))
    v = np.where(known, 0.0, 0.0 if v0 is None else np.asarray(v0, dtype=np.float64))
    a = np.zeros(n)
    out = {k: np.empty((steps + 1, n)) for k in ("u", "v", "a", "f")}
    out["energies"] = np.empty((steps + 1, 3))
    out["min_det"] = np.inf

    def force(w):
        fi, W, det = tl_force(xy, conn, E, nu, t, w)
        out["min_det"] = min(out["min_det"], det)
        return fi, W

    def step(h, load):
        ut = np.where(known, u_in, u + h * v + h * h * 0.5 * a)
        vt = np.where(known, 0.0, v + 0.5 * h * a)
        fi, W = force(ut)
        an = np.where(known, 0.0, (load * f - alpha * (m * vt) - fi) / ((1.0 + 0.5 * h * alpha) * m))
        return ut, vt + 0.5 * h * an, an, fi, W  # (u' = ut: the step's force and energy are the new state's)

    def record(row, fi, W):
        out["u"][row], out["v"][row], out["a"][row] = u, v, a
        out["f"][row] = np.where(known, fi, amp[row] * f)
        out["energies"][row] = 0.5 * v @ (m * v), W, amp[row] * (f @ u)

    u, v, a, fi, W = step(0.0, amp[0])  # (the start is the step with dt = 0)
    record(0, fi, W)
    for i in range(steps):
        u, v, a, fi, W = step(dt, amp[i + 1])
        record(i + 1, fi, W)
    return out
