"""Reference for the transient tests (CPU, scipy; not product): Newmark's method in acceleration form as include/magnetite_hip.h
states it for mag_run_transient, on K and M of tests/modal_ref.py, every solve by one sparse LU factorisation of the step's
matrix (or by a `solver` of the caller's: the stop rule's emulation, the probe's baseline).

  supports   u_P = u_in, v_P = a_P = 0 for all time
  start      M_FF a_0 = (amp[0] f - C v_0 - K u_0)_F,   C = alpha M + eta K
  step       ut = u + dt v + dt^2 (1/2 - beta) a,  vt = v + dt (1 - gamma) a
             A_FF a' = (amp[n+1] f - alpha M vt - K (ut + eta vt))_F,  A = (1 + gamma dt alpha) M + (beta dt^2 + gamma dt eta) K
             u' = ut + beta dt^2 a',  v' = vt + gamma dt a'
  reactions  K (u + eta v) + M (a + alpha v) on P, amp[n] f on F
  energies   T = 1/2 v.Mv,  W = 1/2 u.Ku,  P = amp[n] f_F . u_F"""
import numpy as np
import scipy.sparse.linalg as spla


def lu_solver(A):
    return spla.splu(A.tocsc()).solve


def newmark(K, M, free, u_in, f_in, steps, dt, beta=0.25, gamma=0.5, alpha=0.0, eta=0.0, amplitude=None, u0=None, v0=None,
            solver=lu_solver):
    """dict(u, v, a, f (steps + 1, 2N each), energies (steps + 1, 3 = T, W, P)).  solver(A_FF) returns b -> x."""
    n = K.shape[0]
    known = np.ones(n, dtype=bool)
    known[free] = False
    amp = np.ones(steps + 1) if amplitude is None else np.asarray(amplitude, dtype=np.float64)
    f = np.where(known, 0.0, np.asarray(f_in, dtype=np.float64))
    u = np.where(known, np.asarray(u_in, dtype=np.float64), 0.0 if u0 is None else np.asarray(u0, dtype=np.float64))
    v = np.where(known, 0.0, 0.0 if v0 is None else np.asarray(v0, dtype=np.float64))
    K, M = K.tocsr(), M.tocsr()

    def solve_free(sol, rhs):
        a = np.zeros(n)
        r = rhs[free]
        a[free] = sol(r) if np.any(r != 0.0) else 0.0
        return a

    a = solve_free(solver(M[free][:, free]), amp[0] * f - alpha * (M @ v) - K @ (u + eta * v))
    step = solver(((1.0 + gamma * dt * alpha) * M + (beta * dt * dt + gamma * dt * eta) * K)[free][:, free])
    out = {k: np.empty((steps + 1, n)) for k in ("u", "v", "a", "f")}
    out["energies"] = np.empty((steps + 1, 3))

    def record(row):
        out["u"][row], out["v"][row], out["a"][row] = u, v, a
        out["f"][row] = np.where(known, K @ (u + eta * v) + M @ (a + alpha * v), amp[row] * f)
        out["energies"][row] = 0.5 * v @ (M @ v), 0.5 * u @ (K @ u), amp[row] * (f @ u)

    record(0)
    for i in range(steps):
        ut = np.where(known, u, u + dt * v + dt * dt * (0.5 - beta) * a)
        vt = np.where(known, 0.0, v + dt * (1.0 - gamma) * a)
        a = solve_free(step, amp[i + 1] * f - alpha * (M @ vt) - K @ (ut + eta * vt))
        u, v = ut + beta * dt * dt * a, vt + gamma * dt * a
        record(i + 1)
    return out


class _NodeBlocks:
    """the entries field_cg_ref.inverse_blocks reads of a matrix -- K[2g, 2g], K[2g, 2g + 1], K[2g + 1, 2g + 1] -- of a sparse one"""

    def __init__(self, A):
        self.diagonal, self.above = A.diagonal(), A.diagonal(1)

    def __getitem__(self, ij):
        i, j = ij
        return self.diagonal[i] if i == j else self.above[i]


def cg_solver(known, kind, tol, max_iter=10 ** 7, log=None):
    """A `solver` for newmark(): the pass's own solve, launch by launch -- field_cg_ref.fused_cg (k_cg_field's recurrence) under
    MAG_STOP_REL with `tol`, from zero, on A_FF scattered into the masked 2N x 2N matrix, with the fp32 inverse node blocks of
    kind 2 (Jacobi) / 3 (2x2 blocks); kind 1: plain.  Device `preconditioner` 0 / 1 / 2 is kind 1 / 2 / 3; the CSR phase (cg = 4)
    is plain CG: kind 1.  At the cap the solve hands on its last iterate, x_{max_iter}.  (iterations, converged) of every solve
    is appended to `log`; newmark() does not call the solver for a right-hand side that is exactly zero (0 iterations)."""
    import scipy.sparse as sp

    import field_cg_ref as fc
    known = np.asarray(known) != 0
    n = len(known)
    free = np.flatnonzero(~known)

    def make(A_FF):
        A = A_FF.tocoo()
        Am = sp.csr_matrix((A.data, (free[A.row], free[A.col])), shape=(n, n))
        minv = fc.inverse_blocks(_NodeBlocks(Am), known, kind) if kind >= 2 else None

        def solve(b):
            full = np.zeros(n)
            full[free] = b
            out = fc.fused_cg(Am, full, tol, kind, minv, max_iter=max_iter)
            if log is not None:
                log.append((int(out["iterations"]), int(out["converged"])))
            return out["x"][free]
        return solve
    return make


def moving_start(K, M, free, u_in, f_in, Phi, alpha, eta, amp0=1.0, modes=(1, 2), share=0.5):
    """(u0, v0): a start that every term of M_FF a_0 = (amp[0] f - C v_0 - K u_0)_F feels.  u0 is mode shape Phi[modes[0]] scaled
    so that |(K u0)_F| is `share` of |(amp[0] f - K u_P)_F| (the right-hand side of the start at rest), v0 is Phi[modes[1]] scaled
    so that |(C v0)_F| is the same share of it, C = alpha M + eta K (pass the damped set's coefficients for an undamped run too).
    Every prescribed DOF holds NaN: the header says those entries are ignored."""
    n = K.shape[0]
    known = np.ones(n, dtype=bool)
    known[free] = False
    at_rest = (amp0 * np.where(known, 0.0, f_in) - K @ np.where(known, u_in, 0.0))[free]
    size = share * np.linalg.norm(at_rest)
    u0 = Phi[modes[0]] * (size / np.linalg.norm((K @ Phi[modes[0]])[free]))
    v0 = Phi[modes[1]] * (size / np.linalg.norm((alpha * (M @ Phi[modes[1]]) + eta * (K @ Phi[modes[1]]))[free]))
    u0[known] = v0[known] = np.nan
    return u0, v0


def mode_closed_form(lam, phi, steps, dt):
    """u_n of the undamped average-acceleration scheme (beta 1/4, gamma 1/2) started at rest in mode phi of eigenvalue lam:
    cos(n theta) phi with cos(theta) = (1 - Omega^2 / 4) / (1 + Omega^2 / 4), Omega = sqrt(lam) dt."""
    om2 = lam * dt * dt
    theta = np.arccos((1.0 - om2 / 4.0) / (1.0 + om2 / 4.0))
    return np.cos(np.arange(steps + 1) * theta)[:, None] * phi[None, :]
