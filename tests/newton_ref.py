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
      (an iteration with s < 1 leaves the supports short of lambda u_in: the next one is a first iteration again, on the rest)
    stop, after every update, with the supports in place:  |r_F| <= newton_tol * ref,  ref = max(|lambda f_F|, |f_int(u)_P|)
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
           u0=None, predictor=True, on_factor=None):
    """The loop of mag_run_newton with a sparse LU for the CG: dict(u, f, load, newton_iterations, energies (rows, 2 = W, Pi),
    residuals, step_lengths (one entry per Newton iteration), states (rows, 2N), halvings, converged_increments, converged,
    inverted, min_det, trials).  trials: one tuple per trial state of the run, in order -- (increment, iteration (both from 1), s,
    the smallest det F of the trial, Pi_t - (Pi0 + 1e-4 s g), max(|Pi0|, W), g): what the line search decides on.  iterates: the
    accepted state of every Newton iteration with its smallest det F.  inverted: an accepted state had det F <= 0
    (mag_get_newton_info's [6]).  on_factor(K_FF) is called with every matrix the run factors.
    predictor=False jumps the supports first (the comparison the issue quotes; not the pass's method)."""
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
               min_det=np.inf, trials=[], iterates=[])

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
        pending = True  # (the supports are not at lam u_in yet: until an iteration with s = 1 has moved them)
        for it in range(cap):
            K = tangent(xy, conn, E, nu, t, u)
            dU = np.zeros_like(u)
            if pending:
                dU[known] = lam * u_in[known] - u[known]
                if not predictor:
                    u = u + dU
                    fi, W, det = evaluate(u)
                    K = tangent(xy, conn, E, nu, t, u)
                    dU[:] = 0.0
                    pending = False
            r = np.where(known, 0.0, lam * f - fi - K @ dU)
            du = dU.copy()
            Kff = K[free][:, free].tocsc()
            if on_factor is not None:
                on_factor(Kff)
            du[free] = spla.splu(Kff).solve(r[free])
            slope = float((fi - lam * f) @ du)
            Pi0 = W - lam * float(f @ u)
            s = 1.0
            for h in range(line_search + 1):
                trial = u + s * du
                fi_t, W_t, det_t = evaluate(trial)
                Pi_t = W_t - lam * float(f @ trial)
                energy = slope < 0.0 and abs(s * slope) > 1e-13 * max(abs(Pi0), W) and Pi_t > Pi0 + 1e-4 * s * slope
                out["trials"].append((k + 1, it + 1, s, det_t, Pi_t - (Pi0 + 1e-4 * s * slope), max(abs(Pi0), W), slope))
                if h == line_search or not (det_t <= 0.0 or energy):
                    break
                s *= 0.5
                out["halvings"] += 1
            u, fi, W, det = trial, fi_t, W_t, det_t
            out["iterates"].append((u.copy(), det))
            out["inverted"] = out["inverted"] or det <= 0.0
            rn = np.linalg.norm(np.where(known, 0.0, lam * f - fi))
            ref = max(np.linalg.norm(lam * f), np.linalg.norm(np.where(known, fi, 0.0)))
            out["residuals"].append(rn / ref if ref > 0 else (0.0 if rn == 0 else np.inf))
            out["step_lengths"].append(s)
            pending = pending and s != 1.0
            if rn <= tol * ref and not pending:
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
    return floor_of(case_problem(name, kind), case_run(name, kind, increments)["u"])


def floor_of(p, u, lam=1.0):
    """(u*, lambda_min): three more Newton iterations from the converged u under the load factor lam (the supports stand where u
    has them), and the smallest eigenvalue of K_T,FF(u*)"""
    a = of_problem(p)
    known = np.asarray(p.u_known).reshape(-1) != 0
    free = np.flatnonzero(~known)
    f = np.where(known, 0.0, lam * np.asarray(p.f_in, dtype=np.float64))
    u = np.array(u, dtype=np.float64)
    for _ in range(3):
        fi, _, _ = tl.tl_force(*a, u)
        K = tangent(*a, u)[free][:, free].tocsc()
        u[free] += spla.splu(K).solve((f - fi)[free])
    K = tangent(*a, u)[free][:, free].tocsc()
    lam_min = float(spla.eigsh(K, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    return u, lam_min


def definiteness(A):
    """smallest over largest eigenvalue of a symmetric matrix, dense (the sizes of the tests' small cases)"""
    w = np.linalg.eigvalsh(A.toarray() if sp.issparse(A) else np.asarray(A))
    return float(w[0] / w[-1])


# ---- the cases of tests/test_newton_paths_gpu.py (early ends, the line search's decisions, inversion), admitted on the CPU in
# tests/test_newton.py.  The GPU tests ask the device for the twin's integers, so the load of a case is scanned, as
# transient_tl_cases.FACTOR is, until every converged increment is off the threshold (last <= newton_tol / 10, last-but-one >= 10
# newton_tol), every trial of a search is away from det F = 0 (1e-3) and, where the energy test is live, from its threshold (1e-9
# of max(|Pi0|, W)).  The figures beside a case: last max, last-but-one min; smallest |det F| of a trial, smallest live energy
# margin; smallest eigenvalue ratio of the tangents factored.  At the issue's own loads (beam x 1, plate16 x 64 and x 256, a pull of
# lx) the last-but-one ratio or the energy margin misses its rule (7.0e-10; 9.7e-10, 3.5e-10, 9.5e-11, 4.1e-11).
PATHS = {
    # the beam, three increments, the third one past the cap of 4: 6.2e-12, 5.2e-8; 3.6e-3 at the cap; 1.7e-6
    "early": dict(problem="beam", increments=3, load_factors=(0.125, 0.25, 1.0), max_newton=4),
    # plate16 / load300 x 72, plain Newton through inverted states (10 iterations): 4.1e-15, 1.9e-8; 2.0e-5
    "through": dict(problem="plate16", load_factors=(72.0,)),
    # the same with a search: the inverted trial halves the step twice (1/4, then 1; 7 iterations): 3.8e-14, 6.4e-8; 0.77, 2.8e-9; 7.0e-5
    "inversion72": dict(problem="plate16", load_factors=(72.0,), line_search=8),
    # x 320: three halvings (1/8, then 1; 8 iterations): 3.5e-14, 2.3e-8; 0.46, 1.4e-9; 3.7e-5
    "inversion320": dict(problem="plate16", load_factors=(320.0,), line_search=8),
    # the beam x 1.1 in one increment, the energy rule alone: steps 1/2, 1, 1/2, 1 ... (10 iterations): 1.9e-13, 1.0e-7; 0.95, 1.1e-8; 1.7e-6
    "energy1": dict(problem="beam", load_factors=(1.1,), line_search=1),
    # ... and 1/4, 1 ... (10 iterations, 2 halvings): 1.6e-13, 4.2e-8; 0.95, 3.2e-9; 1.7e-6
    "energy2": dict(problem="beam", load_factors=(1.1,), line_search=2),
    # plate16 pulled by 0.84 lx, a search that never halves (6 iterations, smallest det F 0.90): 5.2e-14, 4.9e-8; 0.90, 2.0e-9; 2.4e-4
    "pull": dict(problem="pull84", line_search=6),
    # ... pulled by 7 lx: the support predictor inverts the part and works against it (g >= 0: no energy test), so the inverted trial
    # alone halves the step, 7 times: steps 1/4, 1/8, 1/4, 1 ... (7 iterations), and the supports arrive over four iterations:
    # 2.7e-14, 1.0e-7; 0.107, 4.0e-9; 2.4e-4
    "pull7": dict(problem="pull700", line_search=8),
}


@functools.lru_cache(maxsize=None)
def path_problem(key):
    which = PATHS[key]["problem"]
    if which == "beam":
        return case_problem("beam", "beam")
    if which == "plate16":
        return case_problem("plate16", "load300")
    from magnetite_amd import meshgen
    mesh = case_problem("plate16", "load300").mesh
    return meshgen.config_fixed_left_pull_right(mesh, delta={"pull84": 0.84, "pull700": 7.0}[which] * np.ptp(mesh.xy[:, 0]))


def path_options(key):
    """the options of the case, as Context.newton and newton() take them"""
    kw = {k: v for k, v in PATHS[key].items() if k != "problem"}
    kw.setdefault("increments", 1)
    if "load_factors" in kw:
        kw["load_factors"] = list(kw["load_factors"])
    return kw


@functools.lru_cache(maxsize=None)
def path_run(key):
    """the twin's run of the case, with out["definite"]: the smallest eigenvalue ratio of the tangents it factors"""
    p = path_problem(key)
    ratios = []
    out = newton(*of_problem(p), p.u_known, p.u_in, p.f_in, on_factor=lambda A: ratios.append(definiteness(A)), **path_options(key))
    out["definite"] = min(ratios)
    return out


@functools.lru_cache(maxsize=None)
def path_floor(key):
    """(u*, lambda_min, ref) of a converged case: floor_of at its last load factor, and the stop rule's ref at u*"""
    p = path_problem(key)
    lam = PATHS[key].get("load_factors", (1.0,))[-1]
    u, lam_min = floor_of(p, path_run(key)["u"], lam)
    known = np.asarray(p.u_known).reshape(-1) != 0
    return u, lam_min, residual(*of_problem(p), known, p.f_in, lam, u)[1]
