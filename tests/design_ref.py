"""Reference for the element stiffness field and the density design update: the numpy twin.

The field: K = sum_e s_e K_e from sensitivities_ref.element_stiffness (the reference's K_e with the signed area), a dense direct
solve, and the passes' references -- sensitivities_ref and adjoint_ref, imported, with s_e applied through a per-element
thickness t s_e (K_e is linear in the thickness).

The design update restates design.hip line by line -- the same operations in the same order, sums over a node's triangles in
the order of its incidence list (ascending element), min / max as fmin / fmax -- so that it differs from the device only in the
order of the volume sum, which `vsum` chooses (numpy.sum, math.fsum)."""
import dataclasses
import functools
import math

import numpy as np

import adjoint_ref as aref
import sensitivities_ref as sref
from magnetite_amd import meshgen

BISECTIONS = 100
DEFAULTS = dict(volume_fraction=0.5, penal=3, scale_min=1e-3, rho_min=1e-3, move=0.2, filter_passes=1)


# ---- the field
def random_scale(E, seed=3):
    """s = 10^U(-2, 0)"""
    return 10.0 ** np.random.default_rng(seed).uniform(-2.0, 0.0, E)


def material(prob):
    return prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness


def scaled_element_stiffness(prob, scale):
    """(E, 6, 6): s_e K_e, and |.| of it for the assembly's error bound"""
    E, nu, t = material(prob)
    return sref.element_stiffness(np.asarray(prob.mesh.xy, dtype=np.float64), np.asarray(prob.mesh.conn), nu, E, t) * np.asarray(scale)[:, None, None]


def dense_K(prob, scale, absolute=False):
    """K = sum_e s_e K_e (2N x 2N, dense); absolute: sum_e s_e |K_e|"""
    conn = np.asarray(prob.mesh.conn)
    ke = scaled_element_stiffness(prob, scale)
    dofs = np.stack([2 * conn, 2 * conn + 1], axis=2).reshape(len(conn), 6)
    n = 2 * len(prob.mesh.xy)
    K = np.zeros((n, n))
    np.add.at(K, (np.repeat(dofs, 6, axis=1).reshape(-1), np.tile(dofs, (1, 6)).reshape(-1)), (np.abs(ke) if absolute else ke).reshape(-1))
    return K


def solve(prob, scale, K=None):
    """numpy_twin.solve's dict (without the stress) for K = sum_e s_e K_e and a direct solve"""
    K = dense_K(prob, scale) if K is None else K
    free, known = np.where(prob.u_known == 0)[0], np.where(prob.u_known == 1)[0]
    Kff = K[np.ix_(free, free)]
    b = prob.f_in[free] - K[np.ix_(free, known)] @ prob.u_in[known]
    u = np.array(prob.u_in, dtype=np.float64)
    u[free] = np.linalg.solve(Kff, b)
    f = np.array(prob.f_in, dtype=np.float64)
    f[known] = K[known] @ u
    return dict(K=K, Kff=Kff, b=b, u=u, f=f, free=free, known=known)


def sensitivities(prob, sol, scale, u_in=None, f_in=None):
    """sensitivities_ref.sensitivities under the field: every element's term carries s_e"""
    E, nu, t = material(prob)
    out = sref.sensitivities(prob.mesh.xy, prob.mesh.conn, prob.u_known, sol["u"], sol["f"], prob.u_in if u_in is None else u_in,
                             prob.f_in if f_in is None else f_in, E, nu, t * np.asarray(scale))
    out["dPi_dt"] = out["strain_energy"] / t
    return out


def adjoint(prob, u, g, scale):
    """adjoint_ref.adjoint under the field, lambda from the direct solve of K_ff lambda_F = g_F with the scaled K"""
    E, nu, t = material(prob)
    lam_sol = solve(dataclasses.replace(prob, u_in=np.zeros_like(prob.u_in), f_in=np.asarray(g, dtype=np.float64)), scale)
    out = aref.adjoint(prob.mesh.xy, prob.mesh.conn, prob.u_known, u, lam_sol["u"], g, lam_sol["f"], E, nu, t * np.asarray(scale))
    out["dJ_dt"] = -out["a"] / t
    return out


def potential(prob, scale):
    """Pi = W - f_F^T u_F at the direct solution under the field, both sums exact"""
    sol = solve(prob, scale)
    E, nu, t = material(prob)
    energy = sref.element_energy(np.asarray(prob.mesh.xy, dtype=np.float64), np.asarray(prob.mesh.conn), sol["u"], nu, E, t * np.asarray(scale))
    free = prob.u_known == 0
    return math.fsum(energy) - math.fsum(prob.f_in[free] * sol["u"][free])


# ---- the meshes of the design tests
def cantilever(mesh, load=-1e6):
    """left edge fixed, a point load fy = load on the node nearest the middle of the right edge"""
    prob = meshgen.config_fixed_left_point_load(mesh, load=0.0)
    prob.f_in[2 * prob.meta["load_node"] + 1] = load
    return prob


TOPOPT_MESHES = {
    "plate_32x16": lambda: meshgen.plate(32, 16, lx=2.0, ly=1.0),
    "frontal16": lambda: meshgen.frontal_like(16),
}


# ---- the design update, as design.hip computes it
class Filter:
    """The one-ring filter F of a mesh and its transpose.  a: signed areas; A: the nodes' area sums; the node sums run over a
    node's triangles in ascending element order, one term after another."""

    def __init__(self, xy, conn):
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        self.conn = conn = np.asarray(conn).reshape(-1, 3)
        x, y = xy[conn][..., 0], xy[conn][..., 1]
        b0, b1, b2 = y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]
        self.area = 0.5 * (x[:, 0] * b0 + x[:, 1] * b1 + x[:, 2] * b2)
        order = np.argsort(conn.reshape(-1), kind="stable")  # (node, 3 e + corner) ascending: the incidence lists
        nodes, elems = conn.reshape(-1)[order], order // 3
        start = np.searchsorted(nodes, np.arange(len(xy) + 1))
        self.rank = np.arange(len(nodes)) - start[nodes]  # position of an entry in its node's list
        self.nodes, self.elems, self.N = nodes, elems, len(xy)
        self.node_area = self.node_sum(self.area)

    def node_sum(self, per_element):
        out = np.zeros(self.N)
        for k in range(int(self.rank.max()) + 1):
            sel = self.rank == k
            out[self.nodes[sel]] += per_element[self.elems[sel]]
        return out

    def forward(self, x):
        with np.errstate(invalid="ignore", divide="ignore"):  # (a node no element touches: never read)
            n = self.node_sum(self.area * x) / self.node_area
        c = self.conn
        return ((n[c[:, 0]] + n[c[:, 1]]) + n[c[:, 2]]) / 3.0

    def transpose(self, y):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = self.node_sum(y / 3.0) / self.node_area
        c = self.conn
        return self.area * ((r[c[:, 0]] + r[c[:, 1]]) + r[c[:, 2]])

    def passes(self, x, P, transpose=False):
        for _ in range(P):
            x = self.transpose(x) if transpose else self.forward(x)
        return np.array(x, dtype=np.float64)


def ipow(x, n):
    """x^n, n >= 0, by repeated multiplication from the left"""
    if n == 0:
        return np.ones_like(x)
    p = x.copy()
    for _ in range(1, n):
        p = p * x
    return p


def oc_update(rho, dJ_drho, w, target, rho_min, move, vsum=np.sum):
    """The optimality-criteria update with the volume constraint: dict(rho, L, bq, reachable, volume)"""
    bq = np.fmax(-dJ_drho, 0.0) / w

    def rho_new(L):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.fmin(np.fmin(1.0, rho + move), np.fmax(np.fmax(rho_min, rho - move), rho * np.sqrt(bq / L)))

    def V(L):
        return float(vsum(w * rho_new(L)))

    lo, hi = 0.0, float(bq.max()) / (rho_min * rho_min)
    reachable = 1 if V(lo) >= target >= V(hi) else 0
    for _ in range(BISECTIONS):
        mid = 0.5 * (lo + hi)
        if V(mid) > target:
            lo = mid
        else:
            hi = mid
    L = 0.5 * (lo + hi)
    new = rho_new(L)
    return dict(rho=new, L=L, bq=bq, reachable=reachable, volume=float(vsum(w * new)))


class Design:
    """mag_design_init / mag_design_step on the host"""

    def __init__(self, xy, conn, volume_fraction=0.5, penal=3, scale_min=1e-3, rho_min=1e-3, move=0.2, filter_passes=1, rho0=None, vsum=np.sum):
        self.filter = Filter(xy, conn)
        self.o = dict(volume_fraction=volume_fraction, penal=penal, scale_min=scale_min, rho_min=rho_min, move=move, filter_passes=filter_passes)
        self.vsum = vsum
        E = len(self.filter.area)
        self.rho = np.full(E, float(volume_fraction)) if rho0 is None else np.array(rho0, dtype=np.float64)
        self.total_area = float(np.sum(self.filter.area))
        self.target = volume_fraction * self.total_area
        self.w = self.filter.passes(self.filter.area, filter_passes, transpose=True)
        self.dJ_drho = np.zeros(E)
        self.interpolate()

    def interpolate(self):
        o = self.o
        self.rho_filtered = self.filter.passes(self.rho, o["filter_passes"])
        self.scale = o["scale_min"] + (1.0 - o["scale_min"]) * ipow(self.rho_filtered, o["penal"])

    def chain(self, dJ_ds):
        o = self.o
        g = ((dJ_ds * (1.0 - o["scale_min"])) * float(o["penal"])) * ipow(self.rho_filtered, o["penal"] - 1)
        return self.filter.passes(g, o["filter_passes"], transpose=True)

    def step(self, dJ_ds=None, energy=None):
        """dJ_ds, or the energies of the run under self.scale (the stiffest design: dJ/ds = -2 energy / s): the info words"""
        if dJ_ds is None:
            dJ_ds = (-2.0 * energy) / self.scale
        self.dJ_drho = self.chain(np.asarray(dJ_ds, dtype=np.float64))
        up = oc_update(self.rho, self.dJ_drho, self.w, self.target, self.o["rho_min"], self.o["move"], self.vsum)
        change = float(np.abs(up["rho"] - self.rho).max())
        self.rho = up["rho"]
        self.interpolate()
        grey = float(np.sum(4.0 * self.rho_filtered * (1.0 - self.rho_filtered)) / len(self.rho))
        return dict(volume_fraction=up["volume"] / self.total_area, lagrange=up["L"], change=change, greyness=grey, reachable=up["reachable"])


def cg_solver(tol):
    """A solve(prob, scale) that runs plain CG on K_ff to |r| <= tol |b| instead of the direct solve (the device's stop rule)"""
    import numpy_twin

    def run(prob, scale):
        K = dense_K(prob, scale)
        free, known = np.where(prob.u_known == 0)[0], np.where(prob.u_known == 1)[0]
        import scipy.sparse as sp
        Kff = sp.csr_matrix(K[np.ix_(free, free)])
        b = prob.f_in[free] - K[np.ix_(free, known)] @ prob.u_in[known]
        x, _, _ = numpy_twin.argmin_cg(Kff, b, tol * float(np.linalg.norm(b)), 200000)
        u = np.array(prob.u_in, dtype=np.float64)
        u[free] = x
        f = np.array(prob.f_in, dtype=np.float64)
        f[known] = K[known] @ u
        return dict(u=u, f=f)

    return run


def topopt(prob, iters=20, solver=solve, **options):
    """Context.topopt on the host: per iteration solve under the design's scale, J = -2 Pi, the energies, one step.
    dict(history: per iteration dict(J, volume_fraction, change, ...); rho, rho_filtered, scale of the final design)"""
    E, nu, t = material(prob)
    xy, conn = np.asarray(prob.mesh.xy, dtype=np.float64), np.asarray(prob.mesh.conn)
    d = Design(xy, conn, **dict(DEFAULTS, **options))
    free = prob.u_known == 0
    history = []
    for _ in range(iters):
        sol = solver(prob, d.scale)
        energy = sref.element_energy(xy, conn, sol["u"], nu, E, t * d.scale)
        J = -2.0 * (float(np.sum(energy)) - float(np.sum(prob.f_in[free] * sol["u"][free])))
        history.append(dict(d.step(energy=energy), J=J))
    return dict(history=history, rho=d.rho, rho_filtered=d.rho_filtered, scale=d.scale)


@functools.lru_cache(maxsize=None)
def reference_trajectory(name, iters=20):
    """The twin's run with direct solves on one of TOPOPT_MESHES under the point load: what the CPU test pins and the GPU
    test compares with"""
    return topopt(cantilever(TOPOPT_MESHES[name]()), iters)


def solver_spread(name, iters=20, tols=(1e-10, 1e-13)):
    """The largest relative difference of J_k between the twin's runs with CG solves at the two tolerances: the round-off and
    solver-tolerance sensitivity of the trajectory (the GPU test's bar on J_k is 100 times this)"""
    prob = cantilever(TOPOPT_MESHES[name]())
    a, b = (np.array([h["J"] for h in topopt(prob, iters, solver=cg_solver(tol))["history"]]) for tol in tols)
    return float(np.abs(a - b).max() / np.abs(b).min()), float((np.abs(a - b) / np.abs(b)).max())


if __name__ == "__main__":
    import time
    for mesh in TOPOPT_MESHES:
        t0 = time.time()
        ref = reference_trajectory(mesh)
        J = np.array([h["J"] for h in ref["history"]])
        print(mesh, "J19/J0", J[-1] / J[0], "largest J[k+1]/J[k]", (J[1:] / J[:-1]).max(),
              "volume error", max(abs(h["volume_fraction"] - 0.5) for h in ref["history"]), "seconds", time.time() - t0)
        t0 = time.time()
        print(mesh, "solver spread of J_k (tol 1e-10 against 1e-13): max |dJ| / min |J|, max relative", solver_spread(mesh), "seconds", time.time() - t0)
