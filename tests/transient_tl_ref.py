"""Reference for the nonlinear transient tests (CPU, numpy / scipy only; not product): Newmark's method in acceleration form on
the total-Lagrangian internal force, every step solved by Newton's method on the consistent tangent, as include/magnetite_hip.h
states it for mag_run_transient_tl -- on newton_ref.tangent, explicit_tl_ref.tl_force and the mass of modal_ref.matrices, with one
sparse LU per Newton iteration in place of the CG.

  supports   u_P = u_in, v_P = a_P = 0 for all time;  C = alpha M
  start      M_FF a_0 = (amp[0] f - alpha M v_0 - f_int(u_0))_F
  step       ut = u + dt v + dt^2 (1/2 - beta) a,  vt = v + dt (1 - gamma) a      (on P: ut = u_in, vt = 0)
             unknown a':  u' = ut + beta dt^2 a',  v' = vt + gamma dt a'
             r(a') = (amp[n+1] f - f_int(u') - M (a' + alpha v'))_F
             Newton:  A_T,FF da = r_F,  A_T = (1 + gamma dt alpha) M + beta dt^2 K_T(u'),  a' += da
             first iterate:  a'_F = (u - ut)_F / (beta dt^2), so that u' = u_n
             stop, after every update:  |r_F| <= newton_tol ref,  ref = max(|amp[n+1] f_F|, |f_int(u')_F|, |(M (a' + alpha v'))_F|)
  reactions  f_int(u) + M (a + alpha v) on P, amp[n] f on F
  energies   T = 1/2 v.Mv,  W = sum_e W_e,  P = amp[n] f_F . u_F"""
import numpy as np
import scipy.sparse.linalg as spla

import explicit_tl_ref as tl
import newton_ref


def newmark_tl(xy, conn, E, nu, t, M, free, u_in, f_in, steps, dt, beta=0.25, gamma=0.5, alpha=0.0, amplitude=None, u0=None, v0=None,
               newton_tol=0.0, max_newton=0, extra=0, start="u", on_factor=None):
    """dict(u, v, a, f (rows, 2N each), energies (rows, 3 = T, W, P), newton_iterations (rows), residuals (one ratio per Newton
    iteration of the run), steps_done, converged, min_det, inverted); rows = steps_done + 1.  inverted: some trial state of the
    run, of a step that did not converge included, had det F <= 0 (mag_get_transient_tl_info's [6]).  on_factor(A_FF) is called
    with every matrix the run factors (M_FF for a_0, then every A_T,FF).  extra = k runs every step k iterations past
    convergence (the round-off floor; newton_iterations and residuals count and hold them).  start: the first iterate of a step --
    "u" (u' = u_n: the pass's), "a" (a' = a_n) or "0" (a' = 0), the two the header warns of."""
    if beta <= 0.0:
        raise ValueError("beta <= 0: the explicit pass")
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

    def force(w):
        fi, W, det = tl.tl_force(xy, conn, E, nu, t, w)
        out["min_det"] = min(out["min_det"], det)
        return fi, W

    def solve_free(A, rhs):
        x = np.zeros(n)
        r = rhs[free]
        if np.any(r != 0.0):
            Aff = A[free][:, free].tocsc()
            if on_factor is not None:
                on_factor(Aff)
            x[free] = spla.splu(Aff).solve(r)
        return x

    def record(row, fi, W):
        out["u"].append(u.copy()), out["v"].append(v.copy()), out["a"].append(a.copy())
        out["f"].append(np.where(known, fi + M @ (a + alpha * v), amp[row] * f))
        out["energies"].append((0.5 * v @ (M @ v), W, amp[row] * (f @ u)))

    fi, W = force(u)
    a = solve_free(M, amp[0] * f - alpha * (M @ v) - fi)
    record(0, fi, W)
    c_u, c_v, c_M = beta * dt * dt, gamma * dt, 1.0 + gamma * dt * alpha
    done = 0
    for i in range(steps):
        ut = np.where(known, u_in, u + dt * v + dt * dt * (0.5 - beta) * a)
        vt = np.where(known, 0.0, v + dt * (1.0 - gamma) * a)
        an = {"u": np.where(known, 0.0, (u - ut) / c_u), "a": a.copy(), "0": np.zeros(n)}[start]
        un, vn = ut + c_u * an, vt + c_v * an
        fi, W = force(un)
        converged, past = False, 0
        for it in range(cap + extra):
            A = c_M * M + c_u * newton_ref.tangent(xy, conn, E, nu, t, un)
            mi = M @ (an + alpha * vn)
            an = an + solve_free(A, np.where(known, 0.0, amp[i + 1] * f - fi - mi))
            un, vn = ut + c_u * an, vt + c_v * an
            fi, W = force(un)
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


def of_problem(prob):
    return newton_ref.of_problem(prob)
