"""Reference for the modal tests (CPU, scipy; not product): K and M of a problem assembled from its triangles, the lowest
eigenpairs of K_FF phi = lambda M_FF phi by shift-invert Lanczos (eigsh, sigma = 0, tol = 0: to round-off), the true relative
residual of a returned pair, and the subspace iteration of mag_run_modal stated in numpy (the prototype the header's algorithm
was tried with; scripts/modal_probe.py drives the same loop through solve_cases as its baseline)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def signed_areas(xy, conn):
    p = np.asarray(xy, dtype=np.float64).reshape(-1, 2)[np.asarray(conn).reshape(-1, 3)]
    x, y = p[..., 0], p[..., 1]
    return 0.5 * (x[:, 0] * (y[:, 1] - y[:, 2]) + x[:, 1] * (y[:, 2] - y[:, 0]) + x[:, 2] * (y[:, 0] - y[:, 1]))


def _dofs(conn):
    """(E, 6): the DOFs of every element, (2 n0, 2 n0 + 1, 2 n1, ...)."""
    conn = np.asarray(conn).reshape(-1, 3).astype(np.int64)
    return np.stack([2 * conn[:, 0], 2 * conn[:, 0] + 1, 2 * conn[:, 1], 2 * conn[:, 1] + 1, 2 * conn[:, 2], 2 * conn[:, 2] + 1], axis=1)


def _assemble(dofs, blocks, n):
    rows = np.repeat(dofs, 6, axis=1).reshape(-1)
    cols = np.tile(dofs, (1, 6)).reshape(-1)
    return sp.csr_matrix((blocks.reshape(-1), (rows, cols)), shape=(n, n))


def stiffness(xy, conn, youngs, nu, t):
    """K (2N x 2N, csr): K_e = B^T D B A t with the SIGNED area A, B's entries divided by 2A (solver.rs:263-331)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    conn = np.asarray(conn).reshape(-1, 3)
    p = xy[conn]
    x, y = p[..., 0], p[..., 1]
    A = signed_areas(xy, conn)
    b = np.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], axis=1)
    g = np.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], axis=1)
    E = len(conn)
    B = np.zeros((E, 3, 6))
    B[:, 0, 0::2] = b
    B[:, 1, 1::2] = g
    B[:, 2, 0::2] = g
    B[:, 2, 1::2] = b
    B /= (2 * A)[:, None, None]
    D = youngs / (1 - nu * nu) * np.array([[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]])
    Ke = np.einsum("eki,kl,elj->eij", B, D, B) * (A * t)[:, None, None]
    return _assemble(_dofs(conn), Ke, 2 * len(xy))


def mass(xy, conn, rho, t, lumped=False):
    """M (2N x 2N, csr): m_e = rho t |A_e|; consistent m_e / 12 [[2,1,1],[1,2,1],[1,1,2]] per direction, or m_e / 3 on each
    corner's diagonal."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    conn = np.asarray(conn).reshape(-1, 3)
    me = rho * t * np.abs(signed_areas(xy, conn))
    node = np.eye(3) / 3 if lumped else (np.ones((3, 3)) + np.eye(3)) / 12
    Me = me[:, None, None] * np.kron(node, np.eye(2))[None]
    return _assemble(_dofs(conn), Me, 2 * len(xy))


def matrices(prob, rho, lumped=False):
    """K, M and the free DOFs of a meshgen.Problem."""
    K = stiffness(prob.mesh.xy, prob.mesh.conn, prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
    M = mass(prob.mesh.xy, prob.mesh.conn, rho, prob.part_thickness, lumped)
    free = np.flatnonzero(np.asarray(prob.u_known) == 0)
    return K, M, free


def eigenpairs(K, M, free, k=8):
    """The k lowest pairs of K_FF phi = lambda M_FF phi: lambda (k,) ascending, Phi (k, 2N) with Phi M Phi^T = I, 0 on P."""
    Kff, Mff = K[free][:, free].tocsc(), M[free][:, free].tocsc()
    n = Kff.shape[0]
    v0 = np.cos(np.arange(n) * 0.7) + 1.5  # (a fixed start vector: the same pairs every time)
    lam, vec = spla.eigsh(Kff, k=k, M=Mff, sigma=0, tol=0, v0=v0)
    order = np.argsort(lam)
    Phi = np.zeros((k, K.shape[0]))
    Phi[:, free] = vec[:, order].T
    return lam[order], Phi


def true_residual(K, M, free, lam, phi):
    """|K_FF phi - lambda M_FF phi| / |lambda M_FF phi|."""
    kp, mp = (K @ phi)[free], lam * (M @ phi)[free]
    return float(np.linalg.norm(kp - mp) / np.linalg.norm(mp))


# ---- the algorithm of mag_run_modal in numpy

def monomial(m):
    """(a, b): the exponents of the m-th monomial xi^a eta^b, by total degree."""
    d = 0
    while (d + 1) * (d + 2) // 2 <= m:
        d += 1
    b = m - d * (d + 1) // 2
    return d - b, b


def start_vectors(xy, u_known, q):
    """(q, 2N): vector j = the (j // 2)-th monomial of the bounding-box-normalised coordinates (shifted by 1/2: no vector
    vanishes on a support line) in direction j % 2, 0 on P."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    xi, eta = (xy[:, 0] - lo[0]) / span[0] + 0.5, (xy[:, 1] - lo[1]) / span[1] + 0.5
    X = np.zeros((q, 2 * len(xy)))
    for j in range(q):
        a, b = monomial(j // 2)
        X[j, (j % 2)::2] = xi ** a * eta ** b
    X[:, np.asarray(u_known) != 0] = 0.0
    return X


def rayleigh_ritz(A, B):
    """The generalised eigenpairs of the symmetric pair (A, B), B positive definite: lambda ascending, Q with Q^T B Q = I."""
    L = np.linalg.cholesky(B)
    Li = np.linalg.inv(L)
    lam, V = np.linalg.eigh(Li @ A @ Li.T)
    return lam, Li.T @ V


def subspace_iteration(K, M, free, X0, p, tol=1e-10, max_outer=50, solve=None):
    """dict(lambda (p), shapes (p, 2N), outer, converged): subspace iteration with the q rows of X0; solve(Y) -> Z with
    K_FF Z = Y on F (default: a sparse LU of K; with a solver of its own K may be None)."""
    n = M.shape[0]
    if solve is None:
        lu = spla.splu(K[free][:, free].tocsc())

        def solve(Y):
            Z = np.zeros_like(Y)
            Z[:, free] = lu.solve(Y[:, free].T).T
            return Z
    mask = np.zeros(n)
    mask[free] = 1.0
    Y = (M @ X0.T).T * mask
    prev, outer, converged = None, 0, 0
    while outer < max_outer:
        Z = solve(Y)
        W = (M @ Z.T).T * mask
        A, B = Z @ Y.T, Z @ W.T
        lam, Q = rayleigh_ritz(0.5 * (A + A.T), 0.5 * (B + B.T))
        X, Y = Q.T @ Z, Q.T @ W
        outer += 1
        if prev is not None and np.max(np.abs(lam[:p] - prev[:p]) / np.abs(lam[:p])) <= tol:
            converged = 1
            break
        prev = lam
    return dict(lam=lam[:p], shapes=X[:p], outer=outer, converged=converged)


@functools.lru_cache(maxsize=None)
def cached(name, rho, lumped=False):
    """(prob, K, M, free, lambda (8), Phi (8, 2N)) of mesh `name` of tests/test_load_cases_gpu.py: computed once, shared, left
    unchanged."""
    from test_load_cases_gpu import MESHES
    prob = MESHES[name][0]()
    K, M, free = matrices(prob, rho, lumped)
    lam, Phi = eigenpairs(K, M, free)
    return prob, K, M, free, lam, Phi
