"""Reference for the explicit-dynamics tests (CPU, numpy only; not product): central differences on the lumped mass as
include/magnetite_hip.h states them for mag_run_explicit, on K and M of modal_ref.matrices(prob, rho, lumped=True); the
Gershgorin bound of the stable step; the closed form of a start at rest in a lumped-mass mode.

  supports   u_P = u_in, v_P = a_P = 0 for all time
  start      a_0 = (amp[0] f - alpha m v_0 - K (u_0 + eta v_0))_F / m
  step       ut = u + dt v + dt^2/2 a,  vt = v + dt/2 a            (on P: ut = u_in, vt = 0)
             a' = (amp[n+1] f - alpha m vt - K (ut + eta vt))_F / ((1 + dt alpha / 2) m),  a'_P = 0
             u' = ut,  v' = vt + dt/2 a'
  reactions  K (u + eta v) + m (a + alpha v) on P, amp[n] f on F
  energies   T = 1/2 v.mv,  W = 1/2 u.Ku,  P = amp[n] f_F . u_F"""
import numpy as np


def explicit(K, M, free, u_in, f_in, steps, dt, alpha=0.0, eta=0.0, amplitude=None, u0=None, v0=None):
    """dict(u, v, a, f (steps + 1, 2N each), energies (steps + 1, 3 = T, W, P)); M: the lumped mass (its diagonal is read)."""
    n = K.shape[0]
    known = np.ones(n, dtype=bool)
    known[free] = False
    m = np.asarray(M.diagonal(), dtype=np.float64)
    amp = np.ones(steps + 1) if amplitude is None else np.asarray(amplitude, dtype=np.float64)
    f = np.where(known, 0.0, np.asarray(f_in, dtype=np.float64))
    u_in = np.asarray(u_in, dtype=np.float64)
    u = np.where(known, u_in, 0.0 if u0 is None else np.asarray(u0, dtype=np.float64))
    v = np.where(known, 0.0, 0.0 if v0 is None else np.asarray(v0, dtype=np.float64))
    a = np.zeros(n)
    K = K.tocsr()
    out = {k: np.empty((steps + 1, n)) for k in ("u", "v", "a", "f")}
    out["energies"] = np.empty((steps + 1, 3))

    def step(h, load):
        ut = np.where(known, u_in, u + h * v + h * h * 0.5 * a)
        vt = np.where(known, 0.0, v + 0.5 * h * a)
        an = np.where(known, 0.0, (load * f - alpha * (m * vt) - K @ (ut + eta * vt)) / ((1.0 + 0.5 * h * alpha) * m))
        return ut, vt + 0.5 * h * an, an

    def record(row):
        out["u"][row], out["v"][row], out["a"][row] = u, v, a
        out["f"][row] = np.where(known, K @ (u + eta * v) + m * (a + alpha * v), amp[row] * f)
        out["energies"][row] = 0.5 * v @ (m * v), 0.5 * u @ (K @ u), amp[row] * (f @ u)

    u, v, a = step(0.0, amp[0])  # (the start is the step with dt = 0)
    record(0)
    for i in range(steps):
        u, v, a = step(dt, amp[i + 1])
        record(i + 1)
    return out


def lambda_bound(K, m, free):
    """max over free DOFs i of (sum over free j of |K_ij|) / m_i: Gershgorin on M_FF^-1 K_FF"""
    Kff = abs(K.tocsr()[free][:, free])
    return float(np.max(np.asarray(Kff.sum(axis=1)).reshape(-1) / np.asarray(m)[free]))


def dt_limit(omega, eta=0.0):
    """the stable step of the scheme for a largest frequency omega: (2 / omega) (sqrt(1 + xi^2) - xi), xi = eta omega / 2 (the
    difference written as 1 / (sqrt(1 + xi^2) + xi): no cancellation)"""
    xi = eta * omega / 2.0
    return (2.0 / omega) / (np.sqrt(1.0 + xi * xi) + xi)


def bound(K, m, free, eta=0.0):
    """dt_bound: dt_limit at omega_bound = sqrt(lambda_bound)"""
    return float(dt_limit(np.sqrt(lambda_bound(K, m, free)), eta))


def omega_max(K, m, free):
    """the true largest frequency of K_FF phi = lambda m phi: Lanczos on the symmetric m^-1/2 K_FF m^-1/2, to round-off"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    s = sp.diags(1.0 / np.sqrt(np.asarray(m)[free]))
    A = (s @ K.tocsr()[free][:, free] @ s).tocsr()
    v0 = np.cos(np.arange(A.shape[0]) * 0.7) + 1.5  # (a fixed start vector)
    return float(np.sqrt(spla.eigsh(A, k=1, which="LA", tol=0, v0=v0, return_eigenvectors=False)[0]))


def mode_closed_form(lam, phi, steps, dt):
    """u_n of the undamped scheme started at rest in the lumped-mass mode phi of eigenvalue lam: cos(n theta) phi with
    cos(theta) = 1 - lam dt^2 / 2"""
    theta = np.arccos(1.0 - lam * dt * dt / 2.0)
    return np.cos(np.arange(steps + 1) * theta)[:, None] * phi[None, :]
