"""Reference for the nonlinear-statics tests (CPU, numpy / scipy only; not product): the consistent tangent of the
total-Lagrangian internal force as include/magnetite_hip.h states it for mag_run_newton, written from the formulas on top of
explicit_tl_ref.strains / tl_force, and the Newton loop of the pass with a sparse direct solve in place of the CG.

  triangle (a, b, c), H, F = I + H and S as in explicit_tl_ref; the reference shape gradients
    g_a = (db.y - dc.y, dc.x - db.x) / 2A,  g_b = (dc.y, -dc.x) / 2A,  g_c = (-db.y, db.x) / 2A;   V = A t
    D = c [[1, nu, 0], [nu, 1, 0], [0, 0, h]],  c = E / (1 - nu^2),  h = (1 - nu) / 2
  K_T[k, l] = V (B_k^T D B_l + (g_k^T S g_l) I),   B_k (3 x 2), column d:  (F_d1 g_k.x,  F_d2 g_k.y,  F_d1 g_k.y + F_d2 g_k.x)

  increment k, lambda = load_factors[k - 1] (k / increments):  f_int(u)_F = lambda f_F,  u_P = lambda u_in
    first iteration    dU_P = lambda u_in - u on P;  K_FF du_F = (lambda f - f_int(u))_F - (K_T dU_P)_F;  u += s (du_F + dU_P)
    later iterations   K_FF du_F = (lambda f - f_int(u))_F;  u += s du_F
    stop, after every update:  |r_F| <= newton_tol * ref,  ref = max(|lambda f_F|, |f_int(u)_P|)
    line search H > 0: s = 1, halved at most H times while the trial state has an element with det F <= 0 or
      Pi(u + s du) > Pi(u) + 1e-4 s g,  Pi = W - lambda f_F.u_F,  g = (f_int(u) - lambda f_F).du  (= -r.du where du_P = 0);
      the energy test is skipped where g >= 0 or |s g| <= 1e-13 max(|Pi|, W)"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import explicit_tl_ref as tl


def shape_gradients(xy, conn):
    """g (E, 3, 2): the reference gradients of the three corners' shape functions"""
    a, b, c = conn[:, 0], conn[:, 1], conn[:, 2]
    db, dc = xy[b] - xy[a], xy[c] - xy[a]
    twoA = db[:, 0] * dc[:, 1] - dc[:, 0] * db[:, 1]
    g = np.empty((conn.shape[0], 3, 2))
    g[:, 0, 0], g[:, 0, 1] = db[:, 1] - dc[:, 1], dc[:, 0] - db[:, 0]
    g[:, 1, 0], g[:, 1, 1] = dc[:, 1], -dc[:, 0]
    g[:, 2, 0], g[:, 2, 1] = -db[:, 1], db[:, 0]
    return g / twoA[:, None, None]


def element_state(xy, conn, E, nu, u):
    """per element: 2A, F (E, 2, 2), (Exx, Eyy, Gxy), (Sxx, Syy, Sxy)"""
    twoA, H, (Exx, Eyy, Gxy) = tl.strains(xy, conn, u)
    c = E / (1.0 - nu * nu)
    S = (c * (Exx + nu * Eyy), c * (Eyy + nu * Exx), c * (1.0 - nu) / 2.0 * Gxy)
    return twoA, H + np.eye(2)[None], (Exx, Eyy, Gxy), S


def tangent(xy, conn, E, nu, t, u):
    """K_T(u) as a scipy CSR matrix (2N x 2N, caller numbering)"""
    xy = np.asarray(xy, dtype=np.float64)
    conn = np.asarray(conn, dtype=np.int64)
    n = 2 * xy.shape[0]
    twoA, F, _, (Sxx, Syy, Sxy) = element_state(xy, conn, E, nu, u)
    g = shape_gradients(xy, conn)
    c = E / (1.0 - nu * nu)
    D = c * np.array([[1.0, nu, 0.0], [nu, 1.0, 0.0], [0.0, 0.0, (1.0 - nu) / 2.0]])
    V = 0.5 * twoA * t
    B = np.empty((conn.shape[0], 3, 3, 2))  # element, corner, strain row, column d
    for k in range(3):
        for d in range(2):
            B[:, k, 0, d] = F[:, d, 0] * g[:, k, 0]
            B[:, k, 1, d] = F[:, d, 1] * g[:, k, 1]
            B[:, k, 2, d] = F[:, d, 0] * g[:, k, 1] + F[:, d, 1] * g[:, k, 0]
    rows, cols, vals = [], [], []
    for k in range(3):
        for l in range(3):
            mat = np.einsum("eid,ij,ejf->edf", B[:, k], D, B[:, l])
            geo = (g[:, k, 0] * (Sxx * g[:, l, 0] + Sxy * g[:, l, 1]) + g[:, k, 1] * (Sxy * g[:, l, 0] + Syy * g[:, l, 1]))
            blk = V[:, None, None] * (mat + geo[:, None, None] * np.eye(2)[None])
            for d in range(2):
                for f in range(2):
                    rows.append(2 * conn[:, k] + d)
                    cols.append(2 * conn[:, l] + f)
                    vals.append(blk[:, d, f])
    K = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return K.tocsr()


def element_rows(xy, conn, E, nu, t, u):
    """(E, 8): Exx, Eyy, Gxy, Sxx, Syy, Sxy, det F, W_e"""
    xy = np.asarray(xy, dtype=np.float64)
    conn = np.asarray(conn, dtype=np.int64)
    twoA, F, (Exx, Eyy, Gxy), (Sxx, Syy, Sxy) = element_state(xy, conn, E, nu, u)
    det = F[:, 0, 0] * F[:, 1, 1] - F[:, 0, 1] * F[:, 1, 0]
    W = 0.5 * twoA * t * (Sxx * Exx + Syy * Eyy + Sxy * Gxy) / 2.0
    return np.stack([Exx, Eyy, Gxy, Sxx, Syy, Sxy, det, W], axis=1)


def residual(xy, conn, E, nu, t, known, f_in, lam, u):
    """(|r_F|, ref, f_int) at u under the load factor lam"""
    fi, _, _ = tl.tl_force(xy, conn, E, nu, t, u)
    f = np.where(known, 0.0, f_in)
    r = np.where(known, 0.0, lam * f - fi)
    ref = max(np.linalg.norm(lam * f), np.linalg.norm(np.where(known, fi, 0.0)))
    return float(np.linalg.norm(r)), float(ref), fi


def newton(xy, conn, E, nu, t, u_known, u_in, f_in, increments=1, load_factors=None, newton_tol=0.0, max_newton=0, line_search=0,
           u0=None, predictor=True):
    """The loop of mag_run_newton with a sparse LU for the CG: dict(u, f, load, newton_iterations, energies (rows, 2 = W, Pi),
    residuals, step_lengths (one entry per Newton iteration), states (rows, 2N), halvings, converged_increments, converged,
    inverted, min_det).  predictor=False jumps the supports first (the comparison the issue quotes; not the pass's method)."""
    xy = np.asarray(xy, dtype=np.float64)
    conn = np.asarray(conn, dtype=np.int64)
    known = np.asarray(u_known).reshape(-1) != 0
    free = np.flatnonzero(~known)
    u_in = np.asarray(u_in, dtype=np.float64).reshape(-1)
    f = np.where(known, 0.0, np.asarray(f_in, dtype=np.float64).reshape(-1))
    tol = newton_tol if newton_tol > 0 else 1e-10
    cap = max_newton if max_newton > 0 else 25
    lams = (np.arange(1, increments + 1) / increments) if load_factors is None else np.asarray(load_factors, dtype=np.float64)
    u = np.zeros(xy.shape[0] * 2) if u0 is None else np.array(u0, dtype=np.float64).reshape(-1)
    out = dict(load=[0.0], newton_iterations=[0], residuals=[], step_lengths=[], states=[u.copy()], halvings=0, inverted=False,
               min_det=np.inf)

    def evaluate(w):
        fi, W, det = tl.tl_force(xy, conn, E, nu, t, w)
        out["min_det"] = min(out["min_det"], det)
        return fi, W, det

    fi, W, det = evaluate(u)
    out["energies"] = [(W, W)]
    done = 0
    for k in range(increments):
        lam = lams[k]
        start = (u.copy(), fi, W)
        converged = False
        for it in range(cap):
            K = tangent(xy, conn, E, nu, t, u)
            dU = np.zeros_like(u)
            if it == 0:
                dU[known] = lam * u_in[known] - u[known]
                if not predictor:
                    u = u + dU
                    fi, W, det = evaluate(u)
                    K = tangent(xy, conn, E, nu, t, u)
                    dU[:] = 0.0
            r = np.where(known, 0.0, lam * f - fi - K @ dU)
            du = dU.copy()
            du[free] = spla.splu(K[free][:, free].tocsc()).solve(r[free])
            slope = float((fi - lam * f) @ du)
            Pi0 = W - lam * float(f @ u)
            s = 1.0
            for h in range(line_search + 1):
                trial = u + s * du
                fi_t, W_t, det_t = evaluate(trial)
                Pi_t = W_t - lam * float(f @ trial)
                energy = slope < 0.0 and abs(s * slope) > 1e-13 * max(abs(Pi0), W) and Pi_t > Pi0 + 1e-4 * s * slope
                if h == line_search or not (det_t <= 0.0 or energy):
                    break
                s *= 0.5
                out["halvings"] += 1
            u, fi, W, det = trial, fi_t, W_t, det_t
            out["inverted"] = out["inverted"] or det <= 0.0
            rn = np.linalg.norm(np.where(known, 0.0, lam * f - fi))
            ref = max(np.linalg.norm(lam * f), np.linalg.norm(np.where(known, fi, 0.0)))
            out["residuals"].append(rn / ref if ref > 0 else (0.0 if rn == 0 else np.inf))
            out["step_lengths"].append(s)
            if rn <= tol * ref:
                converged = True
                out["newton_iterations"].append(it + 1)
                break
        if not converged:
            u, fi, W = start
            break
        done += 1
        out["load"].append(float(lam))
        out["states"].append(u.copy())
        out["energies"].append((W, W - lam * float(f @ u)))
    lam = out["load"][-1]
    out.update(u=u, f=np.where(known, fi, lam * f), converged_increments=done, converged=done == increments,
               residuals=np.array(out["residuals"]), step_lengths=np.array(out["step_lengths"]), states=np.array(out["states"]),
               energies=np.array(out["energies"]), load=np.array(out["load"]), newton_iterations=np.array(out["newton_iterations"]))
    return out


def of_problem(prob):
    """the positional arguments of tangent() / newton() up to t, from a meshgen.Problem"""
    return prob.mesh.xy, prob.mesh.conn, prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness


# ---- the cases of the tests (CPU and GPU), everything computed once, shared, left unchanged
import functools


@functools.lru_cache(maxsize=None)
def case_problem(name, kind):
    """the problem of a case: ("beam", "beam"), or a mesh of explicit_tl_cases.FOUR under "load300" | "pull5" """
    import explicit_tl_cases as cases
    return cases.beam_problem() if kind == "beam" else cases.setup(name, kind)["prob"]


@functools.lru_cache(maxsize=None)
def case_run(name, kind, increments, line_search=0, max_newton=0, newton_tol=0.0):
    """the twin's run of a case"""
    p = case_problem(name, kind)
    return newton(*of_problem(p), p.u_known, p.u_in, p.f_in, increments=increments, line_search=line_search, max_newton=max_newton,
                  newton_tol=newton_tol)


@functools.lru_cache(maxsize=None)
def case_floor(name, kind, increments):
    """u*: the twin's equilibrium run on to its round-off floor (three more iterations at the last load), and the smallest
    eigenvalue of K_T,FF(u*)"""
    p = case_problem(name, kind)
    a = of_problem(p)
    known = np.asarray(p.u_known).reshape(-1) != 0
    free = np.flatnonzero(~known)
    f = np.where(known, 0.0, p.f_in)
    u = case_run(name, kind, increments)["u"].copy()
    for _ in range(3):
        fi, _, _ = tl.tl_force(*a, u)
        K = tangent(*a, u)[free][:, free].tocsc()
        u[free] += spla.splu(K).solve((f - fi)[free])
    K = tangent(*a, u)[free][:, free].tocsc()
    lam_min = float(spla.eigsh(K, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    return u, lam_min
