"""Reference for the material-law tests (CPU, numpy / scipy only; not product): the total-Lagrangian internal force, tangent and
element rows per law as include/magnetite_hip.h states them for mag_set_material_law, and the three loops of the passes (Newton,
explicit, Newmark-Newton) taking the law.

  law "svk"        explicit_tl_ref.tl_force, newton_ref.tangent and newton_ref.element_rows themselves
  law "neo_hooke"  written here in the material form: S and the material tangent DD = 2 dS/dC from W(C), put through B --
                   K_T[k, l] = V (B_k^T DD B_l + (g_k^T S g_l) I) -- where the kernel takes the compact form of the header: the two
                   do not share an algebra slip.  Every formula takes a dtype, so that np.longdouble gives the twin's own round-off
                   (`spread`): the bars of the GPU tests.

    mu = E / (2 (1 + nu)),  Lambda = E nu / ((1 + nu)(1 - 2 nu));  C = I + 2 E_GL,  j2 = det C,  j2m1 = 2 (Exx + Eyy) + 4 Exx Eyy - Gxy^2
    d = C33 - 1 solves g(d) = mu d + Lambda/2 (log1p(j2m1) + log1p(d)) = 0: Newton's method from d0 = min(0, -j2m1 / j2), while the
      iterate still increases (nu < 0: after the first step, while it falls), at most 40 iterations
    S = mu (I - C33 C^-1);  DD = 2 mu C33 (kappa C^-1 (x) C^-1 + I_{C^-1}),  kappa = Lambda / (2 mu C33 + Lambda)
    W_e = V (mu/2 (2 (Exx + Eyy) + d) - mu l + Lambda/2 l^2),  l = ln J = (log1p(j2m1) + log1p(d)) / 2

The loops are restated from newton_ref.newton, explicit_tl_ref.explicit_tl and transient_tl_ref.newmark_tl (those modules cache
their cases per process and stay as they are); with law="svk" they return those twins' results bit for bit (tests/test_hyper.py)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import explicit_tl_ref as tl
import newton_ref

LAWS = ("svk", "neo_hooke")
SOLVE_CAP = 40


def lame(E, nu, dtype=np.float64):
    E, nu = dtype(E), dtype(nu)
    return E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))


def thickness(j2m1, lr, counts=False):
    """d = C33 - 1 per entry of j2m1 under lr = Lambda / mu; with counts also the iterations taken (the moves of the iterate)"""
    j2m1 = np.asarray(j2m1)
    dt = j2m1.dtype.type
    half = dt(0.5) * dt(lr)
    L = np.log1p(j2m1)
    d = np.minimum(dt(0), -j2m1 / (1 + j2m1))
    active = np.ones(d.shape, dtype=bool)
    fell = np.zeros(d.shape, dtype=bool)
    its = np.zeros(d.shape, dtype=np.int64)
    for _ in range(SOLVE_CAP):
        with np.errstate(all="ignore"):
            g = d + half * (L + np.log1p(d))
            dn = d - g / (1 + half / (1 + d))
            rise = active & (dn > d) & ~fell
            fall = active & ~rise & (lr < 0) & (dn < d)
        move = rise | fall
        d = np.where(move, dn, d)
        fell |= fall
        its += move
        active = move
        if not active.any():
            break
    return (d, its) if counts else d


def kinematics(xy, conn, u, dtype=np.float64):
    """explicit_tl_ref.strains in dtype: 2A, H (E, 2, 2), (Exx, Eyy, Gxy)"""
    xy = np.asarray(xy, dtype=dtype)
    U = np.asarray(u, dtype=dtype).reshape(-1, 2)
    a, b, c = conn[:, 0], conn[:, 1], conn[:, 2]
    db, dc = xy[b] - xy[a], xy[c] - xy[a]
    ub, uc = U[b] - U[a], U[c] - U[a]
    twoA = db[:, 0] * dc[:, 1] - dc[:, 0] * db[:, 1]
    H = np.empty((conn.shape[0], 2, 2), dtype=dtype)
    H[:, 0, 0] = (dc[:, 1] * ub[:, 0] - db[:, 1] * uc[:, 0]) / twoA
    H[:, 0, 1] = (db[:, 0] * uc[:, 0] - dc[:, 0] * ub[:, 0]) / twoA
    H[:, 1, 0] = (dc[:, 1] * ub[:, 1] - db[:, 1] * uc[:, 1]) / twoA
    H[:, 1, 1] = (db[:, 0] * uc[:, 1] - dc[:, 0] * ub[:, 1]) / twoA
    Exx = H[:, 0, 0] + (H[:, 0, 0] ** 2 + H[:, 1, 0] ** 2) / 2
    Eyy = H[:, 1, 1] + (H[:, 0, 1] ** 2 + H[:, 1, 1] ** 2) / 2
    Gxy = H[:, 0, 1] + H[:, 1, 0] + H[:, 0, 0] * H[:, 0, 1] + H[:, 1, 0] * H[:, 1, 1]
    return twoA, H, (Exx, Eyy, Gxy)


def neo_state(xy, conn, E, nu, t, u, dtype=np.float64):
    """per element, from W(C): dict(twoA, V, F, strains, d, lj, Ci (C^-1 as (xx, yy, xy)), S (xx, yy, xy), W)"""
    mu, lam = lame(E, nu, dtype)
    twoA, H, (Exx, Eyy, Gxy) = kinematics(xy, conn, u, dtype)
    j2m1 = 2 * (Exx + Eyy) + 4 * Exx * Eyy - Gxy * Gxy
    d = thickness(j2m1, lam / mu)
    with np.errstate(all="ignore"):
        lj = (np.log1p(j2m1) + np.log1p(d)) / 2
        j2 = 1 + j2m1
        Ci = ((1 + 2 * Eyy) / j2, (1 + 2 * Exx) / j2, -Gxy / j2)
    c33 = 1 + d
    S = (mu * (1 - c33 * Ci[0]), mu * (1 - c33 * Ci[1]), mu * (-c33 * Ci[2]))
    V = twoA * dtype(t) / 2
    W = V * (mu / 2 * (2 * (Exx + Eyy) + d) - mu * lj + lam / 2 * lj * lj)
    F = H + np.eye(2, dtype=dtype)[None]
    return dict(twoA=twoA, V=V, F=F, strains=(Exx, Eyy, Gxy), d=d, lj=lj, Ci=Ci, S=S, W=W, mu=mu, lam=lam)


def shape_gradients(xy, conn, dtype=np.float64):
    xy = np.asarray(xy, dtype=dtype)
    a, b, c = conn[:, 0], conn[:, 1], conn[:, 2]
    db, dc = xy[b] - xy[a], xy[c] - xy[a]
    twoA = db[:, 0] * dc[:, 1] - dc[:, 0] * db[:, 1]
    g = np.empty((conn.shape[0], 3, 2), dtype=dtype)
    g[:, 0, 0], g[:, 0, 1] = db[:, 1] - dc[:, 1], dc[:, 0] - db[:, 0]
    g[:, 1, 0], g[:, 1, 1] = dc[:, 1], -dc[:, 0]
    g[:, 2, 0], g[:, 2, 1] = -db[:, 1], db[:, 0]
    return g / twoA[:, None, None]


def neo_force(xy, conn, E, nu, t, u, dtype=np.float64):
    """f_int(u) (2N), W(u), the smallest det F; in dtype"""
    conn = np.asarray(conn, dtype=np.int64)
    st = neo_state(xy, conn, E, nu, t, u, dtype)
    F, (Sxx, Syy, Sxy) = st["F"], st["S"]
    S = np.empty_like(F)
    S[:, 0, 0], S[:, 1, 1], S[:, 0, 1], S[:, 1, 0] = Sxx, Syy, Sxy, Sxy
    P = F @ S
    g = shape_gradients(xy, conn, dtype)
    f = np.zeros((np.asarray(xy).shape[0], 2), dtype=dtype)
    for k in range(3):
        np.add.at(f, conn[:, k], st["V"][:, None] * np.einsum("eij,ej->ei", P, g[:, k]))
    det = F[:, 0, 0] * F[:, 1, 1] - F[:, 0, 1] * F[:, 1, 0]
    W = st["W"].sum()
    return f.reshape(-1), (float(W) if dtype is np.float64 else W), float(det.min())


def neo_blocks(xy, conn, E, nu, t, u, dtype=np.float64):
    """the element tangents (E, 3, 3, 2, 2): block (k, l) of every element, B_k^T DD B_l + (g_k^T S g_l) I times V"""
    conn = np.asarray(conn, dtype=np.int64)
    st = neo_state(xy, conn, E, nu, t, u, dtype)
    F, (Sxx, Syy, Sxy), (cx, cy, cq) = st["F"], st["S"], st["Ci"]
    mu, lam, c33 = st["mu"], st["lam"], 1 + st["d"]
    kappa = lam / (2 * mu * c33 + lam)
    ci = np.stack([cx, cy, cq], axis=1)  # Voigt (11, 22, 12)
    II = np.empty((conn.shape[0], 3, 3), dtype=dtype)  # I_{C^-1}, ijkl = (Ci_ik Ci_jl + Ci_il Ci_jk) / 2
    II[:, 0, 0], II[:, 1, 1], II[:, 2, 2] = cx * cx, cy * cy, (cx * cy + cq * cq) / 2
    II[:, 0, 1] = II[:, 1, 0] = cq * cq
    II[:, 0, 2] = II[:, 2, 0] = cx * cq
    II[:, 1, 2] = II[:, 2, 1] = cy * cq
    DD = (2 * mu * c33)[:, None, None] * (kappa[:, None, None] * ci[:, :, None] * ci[:, None, :] + II)
    g = shape_gradients(xy, conn, dtype)
    B = np.empty((conn.shape[0], 3, 3, 2), dtype=dtype)  # element, corner, strain row (the third: Gxy), column d
    for k in range(3):
        for d in range(2):
            B[:, k, 0, d] = F[:, d, 0] * g[:, k, 0]
            B[:, k, 1, d] = F[:, d, 1] * g[:, k, 1]
            B[:, k, 2, d] = F[:, d, 0] * g[:, k, 1] + F[:, d, 1] * g[:, k, 0]
    blocks = np.empty((conn.shape[0], 3, 3, 2, 2), dtype=dtype)
    eye = np.eye(2, dtype=dtype)[None]
    for k in range(3):
        for l in range(3):
            mat = np.einsum("eid,eij,ejf->edf", B[:, k], DD, B[:, l])
            geo = g[:, k, 0] * (Sxx * g[:, l, 0] + Sxy * g[:, l, 1]) + g[:, k, 1] * (Sxy * g[:, l, 0] + Syy * g[:, l, 1])
            blocks[:, k, l] = st["V"][:, None, None] * (mat + geo[:, None, None] * eye)
    return blocks


def scatter(conn, blocks, num_nodes):
    """the element blocks summed into CSR order: (rowptr, col, val) of the 2N x 2N matrix, val in the blocks' dtype"""
    conn = np.asarray(conn, dtype=np.int64)
    n = 2 * num_nodes
    rows, cols, vals = [], [], []
    for k in range(3):
        for l in range(3):
            for d in range(2):
                for f in range(2):
                    rows.append(2 * conn[:, k] + d), cols.append(2 * conn[:, l] + f), vals.append(blocks[:, k, l, d, f])
    key = np.concatenate(rows) * n + np.concatenate(cols)
    uniq, inv = np.unique(key, return_inverse=True)
    val = np.zeros(uniq.size, dtype=blocks.dtype)
    np.add.at(val, inv, np.concatenate(vals))
    r, c = uniq // n, uniq % n
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, r + 1, 1)
    return np.cumsum(rowptr), c, val


def neo_tangent(xy, conn, E, nu, t, u, dtype=np.float64):
    """K_T(u): a scipy CSR matrix in float64, (rowptr, col, val) in any other dtype"""
    n = np.asarray(xy).shape[0]
    rowptr, col, val = scatter(conn, neo_blocks(xy, conn, E, nu, t, u, dtype), n)
    return sp.csr_matrix((val, col, rowptr), shape=(2 * n, 2 * n)) if dtype is np.float64 else (rowptr, col, val)


def neo_element_rows(xy, conn, E, nu, t, u, dtype=np.float64):
    """(E, 8): Exx, Eyy, Gxy, Sxx, Syy, Sxy, det F, W_e"""
    st = neo_state(xy, np.asarray(conn, dtype=np.int64), E, nu, t, u, dtype)
    F = st["F"]
    det = F[:, 0, 0] * F[:, 1, 1] - F[:, 0, 1] * F[:, 1, 0]
    return np.stack([*st["strains"], *st["S"], det, st["W"]], axis=1)


# ---- per law
def force(law, xy, conn, E, nu, t, u):
    """f_int(u) (2N), W(u), the smallest det F"""
    return tl.tl_force(xy, conn, E, nu, t, u) if law == "svk" else neo_force(xy, conn, E, nu, t, u)


def tangent(law, xy, conn, E, nu, t, u):
    return newton_ref.tangent(xy, conn, E, nu, t, u) if law == "svk" else neo_tangent(xy, conn, E, nu, t, u)


def element_rows(law, xy, conn, E, nu, t, u):
    return newton_ref.element_rows(xy, conn, E, nu, t, u) if law == "svk" else neo_element_rows(xy, conn, E, nu, t, u)


def rows_distance(got, want):
    """the largest entry difference of two sets of element rows over the largest entry of its kind: the strains (columns 0..2),
    the stresses (3..5), det F and W_e.  (Per column a homogeneous state would divide by a stress that vanishes.)"""
    worst = 0.0
    for cols in ((0, 1, 2), (3, 4, 5), (6,), (7,)):
        a, b = np.asarray(got)[:, cols], np.asarray(want)[:, cols]
        big = np.abs(b).max()
        worst = max(worst, float(np.abs(a - b).max() / big) if big > 0 else float(np.abs(a).max()))
    return worst


def spread(xy, conn, E, nu, t, u):
    """the float64 neo-Hooke twin's distance from the same formulas in np.longdouble at u, each over the largest entry:
    dict(force, W, tangent, rows (rows_distance))"""
    LD = np.longdouble
    f, W, _ = neo_force(xy, conn, E, nu, t, u)
    fl, Wl, _ = neo_force(xy, conn, E, nu, t, u, LD)
    K = neo_tangent(xy, conn, E, nu, t, u)
    K.sort_indices()
    _, _, vl = neo_tangent(xy, conn, E, nu, t, u, LD)
    r, rl = neo_element_rows(xy, conn, E, nu, t, u), neo_element_rows(xy, conn, E, nu, t, u, LD)
    return dict(force=float(np.abs(f - fl).max() / np.abs(fl).max()), W=float(abs(W - Wl) / abs(Wl)) if Wl != 0 else 0.0,
                tangent=float(np.abs(K.data - vl).max() / np.abs(vl).max()),
                rows=rows_distance(r, rl))


# ---- the loops, restated with the law
def newton(law, xy, conn, E, nu, t, u_known, u_in, f_in, increments=1, load_factors=None, newton_tol=0.0, max_newton=0, line_search=0,
           u0=None, extra=0):
    """newton_ref.newton (the pass's method: support predictor, stop rule, line search) under `law`; extra = k runs the last
    increment k iterations past convergence (the round-off floor: out["u"] is then u*)"""
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
        fi, W, det = force(law, xy, conn, E, nu, t, w)
        out["min_det"] = min(out["min_det"], det)
        return fi, W, det

    fi, W, det = evaluate(u)
    out["energies"] = [(W, W)]
    done = 0
    for k in range(increments):
        lam = lams[k]
        start = (u.copy(), fi, W)
        converged = False
        pending = True
        past = 0
        more = extra if k == increments - 1 else 0
        for it in range(cap + more):
            K = tangent(law, xy, conn, E, nu, t, u)
            dU = np.zeros_like(u)
            if pending:
                dU[known] = lam * u_in[known] - u[known]
            r = np.where(known, 0.0, lam * f - fi - K @ dU)
            du = dU.copy()
            Kff = K[free][:, free].tocsc()
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
            if converged:
                past += 1
            elif rn <= tol * ref and not pending:
                converged = True
                out["newton_iterations"].append(it + 1)
            elif it + 1 >= cap:
                break
            if converged and past == more:
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


def explicit_tl(law, xy, conn, E, nu, t, M, free, u_in, f_in, steps, dt, alpha=0.0, amplitude=None, u0=None, v0=None, dtype=np.float64):
    """explicit_tl_ref.explicit_tl under `law`; dtype=np.longdouble (neo-Hooke): the same loop in extended precision, the
    measure of the float64 run's own round-off"""
    n = 2 * np.asarray(xy).shape[0]
    known = np.ones(n, dtype=bool)
    known[free] = False
    m = np.asarray(M.diagonal(), dtype=dtype)
    amp = np.ones(steps + 1, dtype=dtype) if amplitude is None else np.asarray(amplitude, dtype=dtype)
    f = np.where(known, 0.0, np.asarray(f_in, dtype=dtype))
    u_in = np.asarray(u_in, dtype=dtype)
    u = np.where(known, u_in, 0.0 if u0 is None else np.asarray(u0, dtype=dtype))
    v = np.where(known, 0.0, 0.0 if v0 is None else np.asarray(v0, dtype=dtype))
    a = np.zeros(n, dtype=dtype)
    dt, alpha = dtype(dt), dtype(alpha)
    out = {k: np.empty((steps + 1, n), dtype=dtype) for k in ("u", "v", "a", "f")}
    out["energies"] = np.empty((steps + 1, 3), dtype=dtype)
    out["min_det"] = np.inf

    def evaluate(w):
        fi, W, det = force(law, xy, conn, E, nu, t, w) if dtype is np.float64 else neo_force(xy, conn, E, nu, t, w, dtype)
        out["min_det"] = min(out["min_det"], det)
        return fi, W

    def step(h, load):
        ut = np.where(known, u_in, u + h * v + h * h * 0.5 * a)
        vt = np.where(known, 0.0, v + 0.5 * h * a)
        fi, W = evaluate(ut)
        an = np.where(known, 0.0, (load * f - alpha * (m * vt) - fi) / ((1.0 + 0.5 * h * alpha) * m))
        return ut, vt + 0.5 * h * an, an, fi, W

    def record(row, fi, W):
        out["u"][row], out["v"][row], out["a"][row] = u, v, a
        out["f"][row] = np.where(known, fi, amp[row] * f)
        out["energies"][row] = 0.5 * v @ (m * v), W, amp[row] * (f @ u)

    u, v, a, fi, W = step(0.0, amp[0])
    record(0, fi, W)
    for i in range(steps):
        u, v, a, fi, W = step(dt, amp[i + 1])
        record(i + 1, fi, W)
    return out


def newmark_tl(law, xy, conn, E, nu, t, M, free, u_in, f_in, steps, dt, beta=0.25, gamma=0.5, alpha=0.0, amplitude=None, u0=None, v0=None,
               newton_tol=0.0, max_newton=0, extra=0):
    """transient_tl_ref.newmark_tl (first iterate u' = u_n) under `law`"""
    xy = np.asarray(xy, dtype=np.float64)
    conn = np.asarray(conn, dtype=np.int64)
    n = 2 * xy.shape[0]
    known = np.ones(n, dtype=bool)
    known[free] = False
    tol = newton_tol if newton_tol > 0 else 1e-10
    cap = max_newton if max_newton > 0 else 25
    amp = np.ones(steps + 1) if amplitude is None else np.asarray(amplitude, dtype=np.float64)
    f = np.where(known, 0.0, np.asarray(f_in, dtype=np.float64))
    u_in = np.asarray(u_in, dtype=np.float64)
    u = np.where(known, u_in, 0.0 if u0 is None else np.asarray(u0, dtype=np.float64))
    v = np.where(known, 0.0, 0.0 if v0 is None else np.asarray(v0, dtype=np.float64))
    M = M.tocsr()
    out = dict(u=[], v=[], a=[], f=[], energies=[], newton_iterations=[0], residuals=[], min_det=np.inf)

    def evaluate(w):
        fi, W, det = force(law, xy, conn, E, nu, t, w)
        out["min_det"] = min(out["min_det"], det)
        return fi, W

    def solve_free(A, rhs):
        x = np.zeros(n)
        r = rhs[free]
        if np.any(r != 0.0):
            x[free] = spla.splu(A[free][:, free].tocsc()).solve(r)
        return x

    def record(row, fi, W):
        out["u"].append(u.copy()), out["v"].append(v.copy()), out["a"].append(a.copy())
        out["f"].append(np.where(known, fi + M @ (a + alpha * v), amp[row] * f))
        out["energies"].append((0.5 * v @ (M @ v), W, amp[row] * (f @ u)))

    fi, W = evaluate(u)
    a = solve_free(M, amp[0] * f - alpha * (M @ v) - fi)
    record(0, fi, W)
    c_u, c_v, c_M = beta * dt * dt, gamma * dt, 1.0 + gamma * dt * alpha
    done = 0
    for i in range(steps):
        ut = np.where(known, u_in, u + dt * v + dt * dt * (0.5 - beta) * a)
        vt = np.where(known, 0.0, v + dt * (1.0 - gamma) * a)
        an = np.where(known, 0.0, (u - ut) / c_u)
        un, vn = ut + c_u * an, vt + c_v * an
        fi, W = evaluate(un)
        converged, past = False, 0
        for it in range(cap + extra):
            A = c_M * M + c_u * tangent(law, xy, conn, E, nu, t, un)
            mi = M @ (an + alpha * vn)
            an = an + solve_free(A, np.where(known, 0.0, amp[i + 1] * f - fi - mi))
            un, vn = ut + c_u * an, vt + c_v * an
            fi, W = evaluate(un)
            mi = M @ (an + alpha * vn)
            rn = np.linalg.norm(np.where(known, 0.0, amp[i + 1] * f - fi - mi))
            ref = max(np.linalg.norm(amp[i + 1] * f), np.linalg.norm(np.where(known, 0.0, fi)), np.linalg.norm(np.where(known, 0.0, mi)))
            out["residuals"].append(rn / ref if ref > 0 else (0.0 if rn == 0 else np.inf))
            if converged:
                past += 1
            elif rn <= tol * ref:
                converged = True
            elif it + 1 >= cap:
                break
            if converged and past == extra:
                break
        if not converged:
            break
        out["newton_iterations"].append(it + 1)
        u, v, a = un, vn, an
        record(i + 1, fi, W)
        done += 1
    for k in ("u", "v", "a", "f", "energies", "residuals", "newton_iterations"):
        out[k] = np.array(out[k])
    out.update(steps_done=done, converged=done == steps, inverted=bool(out["min_det"] <= 0.0))
    return out


# ---- the cases of the tests (CPU and GPU), everything computed once, shared, left unchanged
NU_STRIP = 0.33


@functools.lru_cache(maxsize=None)
def strip_problem(stretch=0.5, nu=NU_STRIP):
    """plate(8, 4, lx=1, ly=0.5): the left edge held in x, the right edge moved to stretch * lx, the bottom edge on rollers (held
    in y) -- a homogeneous uniaxial state"""
    from magnetite_amd import meshgen
    mesh = meshgen.plate(8, 4, lx=1.0, ly=0.5)
    x, y = mesh.xy[:, 0], mesh.xy[:, 1]
    known = np.zeros((mesh.num_nodes, 2), dtype=np.uint8)
    u_in = np.zeros((mesh.num_nodes, 2))
    left, right, bottom = x < x.min() + 1e-9, x > x.max() - 1e-9, y < y.min() + 1e-9
    known[left, 0] = known[right, 0] = 1
    known[bottom, 1] = 1
    u_in[right, 0] = (stretch - 1.0) * (x.max() - x.min())
    return meshgen.Problem(mesh, known.reshape(-1), u_in.reshape(-1), np.zeros(2 * mesh.num_nodes), poisson_ratio=nu)


def of_problem(p):
    return newton_ref.of_problem(p)


@functools.lru_cache(maxsize=None)
def case_problem(name, kind):
    """newton_ref.case_problem's, and ("strip", "strip"): the strip squeezed to half its length"""
    return strip_problem() if kind == "strip" else newton_ref.case_problem(name, kind)


@functools.lru_cache(maxsize=None)
def case_run(law, name, kind, increments, line_search=0, extra=0):
    p = case_problem(name, kind)
    return newton(law, *of_problem(p), p.u_known, p.u_in, p.f_in, increments=increments, line_search=line_search, extra=extra)


def finite_state(p, scale=0.05, seed=3):
    """a smooth finite state of the mesh, strains of the order of `scale`: a shear, a stretch and a bend"""
    xy = p.mesh.xy
    d = (xy - xy.mean(axis=0)) / np.ptp(xy, axis=0).max()
    rng = np.random.default_rng(seed)
    A = scale * rng.uniform(-1.0, 1.0, (2, 2))
    q = scale * rng.uniform(-1.0, 1.0, 2)
    u = d @ A.T + np.stack([q[0] * d[:, 1] ** 2, q[1] * d[:, 0] ** 2], axis=1)
    return (u * np.ptp(xy, axis=0).max()).reshape(-1)
