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

PIVOT_TOL = 1e-13  # kEigPivotTol of csrc/modal_host.h
_MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(z):
    """the finaliser of splitmix64 on an array of uint64 (the arithmetic wraps)"""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_unit(xy, c):
    """(N,) in [-1, 1): the start value of stream c at every node, a fixed integer hash of the bits of the node's coordinates
    (+ 0.0: a -0 counts as 0) and of c -- k_modal_start's twin, bit for bit."""
    xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2) + 0.0)
    bits = xy.view(np.uint64)
    golden = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        k = _mix(bits[:, 0] + golden)
        k = _mix(k ^ bits[:, 1])
        k = _mix(k + np.uint64(c + 1) * golden)
    return (k >> np.uint64(11)).astype(np.float64) / 4503599627370496.0 - 1.0


def start_vectors(xy, u_known, q):
    """(q, 2N): DOF d of node i in vector j = hash_unit(xy, 2 j + d)[i], 0 on P: of the size of 1 everywhere, independent on
    any mesh (no polynomial of the coordinates: nothing degenerates on a strip one element thick), a function of the
    coordinates and j only."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    X = np.zeros((q, 2 * len(xy)))
    for j in range(q):
        X[j, 0::2] = hash_unit(xy, 2 * j)
        X[j, 1::2] = hash_unit(xy, 2 * j + 1)
    X[:, np.asarray(u_known) != 0] = 0.0
    return X


class Dependent(Exception):
    """the refusal of sym_def_eig (EIG_DEPENDENT): .pivot = the smallest figure seen"""

    def __init__(self, pivot):
        super().__init__("dependent vectors: pivot figure %g <= %g" % (pivot, PIVOT_TOL))
        self.pivot = pivot


def rayleigh_ritz(A, B, pivot_tol=PIVOT_TOL):
    """(lambda ascending, Q with Q^T B Q = I, pivot) of the symmetric positive definite pair (A, B) by the device's rule
    (csrc/modal_host.h): A scaled to a unit diagonal and factored, A_s = L L^T -- A = Z^T K Z carries lambda_q / lambda_1 where
    B = Z^T M Z carries its square --, mu = the eigenvalues of L^-1 B_s L^-T, lambda = 1 / mu.  pivot = the smallest of the
    Cholesky pivots (each against its own unit diagonal) and of mu_min / mu_max; at or below pivot_tol: Dependent."""
    n = len(A)
    dA = np.diag(A)
    if not np.all(dA > 0):
        raise Dependent(float(dA.min()))
    d = 1.0 / np.sqrt(dA)
    As, Bs = A * np.outer(d, d), B * np.outer(d, d)
    L = np.zeros((n, n))
    pivot = np.inf
    for j in range(n):
        s = As[j, j] - L[j, :j] @ L[j, :j]
        pivot = min(pivot, float(s))
        if not s > pivot_tol:
            raise Dependent(float(s))
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (As[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Li = np.linalg.inv(L)
    C = Li @ Bs @ Li.T
    mu, V = np.linalg.eigh(0.5 * (C + C.T))
    mu, V = mu[::-1], V[:, ::-1]
    pivot = min(pivot, float(mu[-1] / mu[0]))
    if not mu[-1] > pivot_tol * mu[0]:
        raise Dependent(float(mu[-1] / mu[0]))
    return 1.0 / mu, (d[:, None] * (Li.T @ V)) / np.sqrt(mu)[None, :], pivot


def subspace_iteration(K, M, free, X0, p, tol=1e-10, max_outer=50, solve=None, pivot_tol=PIVOT_TOL):
    """dict(lam (p), shapes (p, 2N), outer, converged, pivots (one figure of rayleigh_ritz per step), refused): subspace
    iteration with the q rows of X0; solve(Y) -> Z with K_FF Z = Y on F (default: a sparse LU of K; with a solver of its own K
    may be None).  A step that the device's pivot rule refuses ends the loop: refused = that step (from 1), else 0."""
    n = M.shape[0]
    if solve is None:
        lu = spla.splu(K[free][:, free].tocsc())

        def solve(Y):
            Z = np.zeros_like(Y)
            Z[:, free] = lu.solve(Y[:, free].T).T
            return Z
    mask = np.zeros(n)
    mask[free] = 1.0
    X = X0
    Y = (M @ X0.T).T * mask
    lam = np.full(len(X0), np.nan)
    prev, outer, converged, pivots, refused = None, 0, 0, [], 0
    while outer < max_outer:
        Z = solve(Y)
        W = (M @ Z.T).T * mask
        A, B = Z @ Y.T, Z @ W.T
        try:
            lam, Q, pivot = rayleigh_ritz(0.5 * (A + A.T), 0.5 * (B + B.T), pivot_tol)
        except Dependent as e:
            pivots.append(e.pivot)
            refused = outer + 1
            break
        pivots.append(pivot)
        X, Y = Q.T @ Z, Q.T @ W
        outer += 1
        if prev is not None and np.max(np.abs(lam[:p] - prev[:p]) / np.abs(lam[:p])) <= tol:
            converged = 1
            break
        prev = lam
    return dict(lam=lam[:p], shapes=X[:p], outer=outer, converged=converged, pivots=pivots, refused=refused)


# ---- the parts of the modal tests by name

def _cantilever(*args, **kw):
    from magnetite_amd import meshgen
    return meshgen.config_fixed_left_point_load(meshgen.plate(*args, **kw))


def _clamped_plate():
    """plate(16) with every boundary node held in both directions"""
    from magnetite_amd import meshgen
    prob = meshgen.config_fixed_left_pull_right(meshgen.plate(16))
    x, y = prob.mesh.xy[:, 0], prob.mesh.xy[:, 1]
    edge = (x == x.min()) | (x == x.max()) | (y == y.min()) | (y == y.max())
    known = np.zeros((prob.mesh.num_nodes, 2), dtype=np.uint8)
    known[edge] = 1
    prob.u_known = known.reshape(-1)
    prob.u_in = np.zeros(known.size)
    prob.f_in = np.zeros(known.size)
    return prob


def _mesh(name):
    """a mesh of tests/test_load_cases_gpu.py"""
    def make():
        from test_load_cases_gpu import MESHES
        return MESHES[name][0]()
    return make


PARTS = {
    "plate16": _mesh("plate16"), "holes3k": _mesh("holes3k"), "frontal3k": _mesh("frontal3k"), "two_fans": _mesh("two_fans"),
    "beam16": lambda: _cantilever(64, 4, lx=16.0, ly=1.0),   # 16:1, 325 nodes
    "beam8": lambda: _cantilever(64, 8, lx=8.0, ly=1.0),     # 8:1, 585 nodes
    "bar4": lambda: _cantilever(32, 8, lx=4.0, ly=1.0),      # 4:1, 297 nodes
    "strip": lambda: _cantilever(32, 1, lx=8.0, ly=0.25),    # one element thick: eta takes two values
    "clamped16": _clamped_plate,
}


@functools.lru_cache(maxsize=None)
def cached(name, rho, lumped=False, k=8):
    """(prob, K, M, free, lambda (k), Phi (k, 2N)) of part `name` of PARTS: computed once, shared, left unchanged."""
    prob = PARTS[name]()
    K, M, free = matrices(prob, rho, lumped)
    lam, Phi = eigenpairs(K, M, free, k)
    return prob, K, M, free, lam, Phi
