"""numpy twin of the fp32 CG leg (mag_options.precision = 1, cg_kernel == 4): the owner-computes operator of fan_force and
the fused iteration's recurrence, with every quantity held in a chosen dtype.  In float64 it is one more restatement of
the reference (checked against numpy_twin and the oracle in test_fp32_twin.py); in float32 it is a FAMILY of legitimate
realisations -- element order permuted, coordinate origin anywhere in the bounding box -- whose spread around the fp64
answer is what the GPU tests take their bars from: the kernel is one more member (its own ring order, explicit FMAs,
1.0f / a), so it has to land within a small multiple of that spread.  The code under test never supplies a bar.

Numpy only: nothing here touches the GPU or the C oracle.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
STOP_RNORM, STOP_RNORM_SQ, STOP_REL = 0, 1, 2


def apply(problem, dtype=np.float64, origin=None, element_perm=None, cast_first=False):
    """v -> K v with the rows of prescribed DOFs zeroed, as k_cg_fused32 forms it: every element contributes to each of its
    three corners a from differences relative to that corner (d = c - c_a, u = v - v_a; cg_device.h fan_force), coordinates
    are (xy - origin) cast to dtype, contributions are accumulated in dtype in the order of element_perm.
    cast_first=True is a seeded ERROR for the power tests: coordinates cast to dtype before the origin is subtracted."""
    dt = np.dtype(dtype).type
    xy = np.asarray(problem.mesh.xy, dtype=np.float64)
    conn = np.asarray(problem.mesh.conn, dtype=np.int64)
    if element_perm is not None:
        conn = conn[np.asarray(element_perm)]
    o = xy.min(axis=0) if origin is None else np.asarray(origin, dtype=np.float64)
    X = (xy.astype(dtype) - o.astype(dtype)) if cast_first else (xy - o).astype(dtype)
    E, nu, t = float(problem.youngs_modulus), float(problem.poisson_ratio), float(problem.part_thickness)
    c0, nuf, h = dt(E * t / (2.0 * (1.0 - nu * nu))), dt(nu), dt((1.0 - nu) / 2.0)
    # the three corners of every element, element-major: (a, b, c) cyclic, so the orientation (sign of 2A) is the element's
    a = conn.reshape(-1)
    b = conn[:, [1, 2, 0]].reshape(-1)
    c = conn[:, [2, 0, 1]].reshape(-1)
    db, dc = X[b] - X[a], X[c] - X[a]
    ba, ga = db[:, 1] - dc[:, 1], dc[:, 0] - db[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = c0 / (db[:, 0] * dc[:, 1] - dc[:, 0] * db[:, 1])
    keep = (np.asarray(problem.u_known).reshape(-1, 2) == 0).astype(dtype)
    n = xy.shape[0]

    def K(v):
        V = np.asarray(v, dtype=dtype).reshape(-1, 2)
        ub, uc = V[b] - V[a], V[c] - V[a]
        ex = dc[:, 1] * ub[:, 0] - db[:, 1] * uc[:, 0]
        ey = db[:, 0] * uc[:, 1] - dc[:, 0] * ub[:, 1]
        g = (dc[:, 1] * ub[:, 1] - dc[:, 0] * ub[:, 0]) + (db[:, 0] * uc[:, 0] - db[:, 1] * uc[:, 1])
        sx, sy, tq = nuf * ey + ex, nuf * ex + ey, h * g
        out = np.zeros((n, 2), dtype=dtype)
        np.add.at(out[:, 0], a, w * (ba * sx + ga * tq))
        np.add.at(out[:, 1], a, w * (ga * sy + ba * tq))
        return (out * keep).reshape(-1)

    return K


def cg(apply_fn, b, dtype=np.float64, max_iter=10 ** 7, stop_mode=STOP_RNORM, tol=1e-4, hist_len=None):
    """The recurrence of the fused iteration kernel (cg.hip, fused_step + k_cg_fused32), launch for launch: r = -b,
    p = beta p - r, x += alpha p; the four dots {r.r, p.q, r.q, q.q} in float64 from the dtype vectors;
    alpha = rr / pq, beta = (rr + 2 alpha rq + alpha^2 qq) / rr, both cast to dtype; cost, stop rule, iteration cap and
    argmin's best_param (the lowest-cost iterate) as fused_step records them.
    b is the right-hand side over ALL DOFs (zero on prescribed ones).  Returns dict(x, iterations, best_iteration,
    converged, final_cost, history, alphas)."""
    dt = np.dtype(dtype).type
    r = -np.asarray(b, dtype=np.float64).astype(dtype)
    q, p, x = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    f64 = lambda v: v.astype(np.float64)
    bb = float(f64(r) @ f64(r))
    S = (bb, 1.0, 0.0, 0.0)
    target = tol * np.sqrt(bb) if stop_mode == STOP_REL else tol
    hist, alphas = [], []
    best, best_iter, x_best = np.inf, 0, x.copy()
    if bb == 0.0:
        return dict(x=f64(x), iterations=0, best_iteration=0, converged=True, final_cost=0.0, history=np.array(hist),
                    alphas=np.array(alphas))
    j, converged = 0, False
    while True:
        rr = S[0]
        cost = abs(rr) if stop_mode == STOP_RNORM_SQ else float(np.sqrt(rr))
        done = j - 1
        if done >= 1:
            hist.append(cost)
            if cost < best:
                best, best_iter, x_best = cost, done, x.copy()
        converged = done >= 1 and cost <= target
        if converged or not np.isfinite(rr) or done >= max_iter:
            break
        alpha = rr / S[1]
        beta = (alpha * alpha * S[3] + (2.0 * alpha * S[2] + rr)) / rr
        al, be = dt(alpha), dt(beta)
        if j >= 1:
            alphas.append(float(al))
        r = r + al * q
        x = x + al * p
        p = be * p - r
        q = apply_fn(p)
        R, P, Q = f64(r), f64(p), f64(q)
        S = (float(R @ R), float(P @ Q), float(R @ Q), float(Q @ Q))
        j += 1
    iters = max(j - 1, 0)
    h = np.array(hist if hist_len is None else hist[:hist_len])
    return dict(x=f64(x_best), iterations=iters, best_iteration=best_iter, converged=bool(converged), final_cost=cost,
                history=h, alphas=np.array(alphas))


def family(problem, n=8, seed=0):
    """n float32 realisations as (origin, element_perm): variant 0 is mesh order with the bounding-box corner, the others a
    seeded element permutation and a seeded origin inside the bounding box (the kernel's origin is its tile's first node)."""
    rng = np.random.default_rng(seed)
    xy = np.asarray(problem.mesh.xy, dtype=np.float64)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    E = problem.mesh.num_elements
    out = [(lo.copy(), np.arange(E))]
    for _ in range(n - 1):
        out.append((lo + rng.random(2) * (hi - lo), rng.permutation(E)))
    return out


def family_applies(problem, n=8, seed=0, dtype=np.float32):
    return [apply(problem, dtype, origin=o, element_perm=perm) for o, perm in family(problem, n, seed)]


def rhs(problem, K_matvec):
    """b over all DOFs (float64): f_in - K u_known on the free DOFs, zero on the prescribed ones (solver.rs:365-404)"""
    known = np.asarray(problem.u_known) == 1
    b = np.where(known, 0.0, problem.f_in)
    if np.any(problem.u_in[known] != 0.0):
        b = b - np.where(known, 0.0, K_matvec(np.where(known, problem.u_in, 0.0)))
    return b


def fit(u1, u2, b, q_ref, free):
    """Least-squares coefficients (c1, c2) of d = u(max_iter=2) - u(max_iter=1) on {b, q_ref} over the free DOFs, and
    alpha_1 = (x1.b) / (b.b)"""
    d = (np.asarray(u2, dtype=np.float64) - np.asarray(u1, dtype=np.float64))[free]
    A = np.stack([b[free], q_ref[free]], axis=1)
    scale = np.abs(A).max(axis=0)
    c = np.linalg.lstsq(A / scale, d, rcond=None)[0] / scale
    alpha1 = float(np.asarray(u1, dtype=np.float64)[free] @ b[free]) / float(b[free] @ b[free])
    return d, c, alpha1


def probe_ratio(u1, u2, b, q_ref, Kabs_b, free):
    """max over free DOFs i of |d - c1 b - c2 q_ref|_i / (eps32 (|c1||b_i| + |c2|(|K||b|)_i + |x2_i|)): the entry-wise
    distance of the fp32 operator from K, in units of its float32 rounding.  A DOF whose denominator is zero (a node no
    element uses, no load) must come back exactly zero.  Returns (ratio, alpha1)."""
    d, (c1, c2), alpha1 = fit(u1, u2, b, q_ref, free)
    num = np.abs(d - c1 * b[free] - c2 * q_ref[free])
    den = EPS32 * (abs(c1) * np.abs(b[free]) + abs(c2) * Kabs_b[free] + np.abs(np.asarray(u2, dtype=np.float64)[free]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(den > 0.0, num / den, np.where(num == 0.0, 0.0, np.inf))
    return float(ratio.max()), alpha1


def history_dev(h, h64):
    """per iteration |h / h64 - 1|"""
    n = min(len(h), len(h64))
    return np.abs(np.asarray(h[:n], dtype=np.float64) / np.asarray(h64[:n], dtype=np.float64) - 1.0)


def solve(problem, apply_fn, b, dtype, **kw):
    """u over all DOFs: prescribed values untouched, the CG iterate on the free ones"""
    s = cg(apply_fn, b, dtype, **kw)
    known = np.asarray(problem.u_known) == 1
    s["u"] = np.where(known, problem.u_in, s["x"])
    return s
