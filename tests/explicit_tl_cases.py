"""The cases of the total-Lagrangian explicit-dynamics tests (CPU and GPU), everything computed once, shared, left unchanged.

  load300  the four meshes of explicit_cases.FOUR under config_fixed_left_point_load(mesh, load=3e8), a step load, 256 steps
  pull5    the same meshes under config_fixed_left_pull_right(mesh, delta=0.05 lx), started from u0_x = 0.05 (x - x_min),
           u0_y = 0, 256 steps; undamped, and under rayleigh = (0.05 * 2 pi * 1000, 0) ("pull5d")
  beam     plate(32, 4, lx=1.0, ly=0.125), left edge fixed, fy = -6e6 / 5 on each of the five right-edge nodes, 1479 steps:
           half the first period at 0.9 dt_bound; the tip moves 0.52 L

Every case is finite over its steps at 0.9 dt_bound and its smallest det F is between 0.83 and 1.01; the total-Lagrangian and
the linear answers are 8e-3 to 0.29 apart (tests/test_explicit_tl.py checks both on the cheapest cases)."""
import functools

import numpy as np

import explicit_cases
import explicit_ref
import explicit_tl_ref as ref
import modal_ref
from magnetite_amd import meshgen

RHO = explicit_cases.RHO
FOUR = explicit_cases.FOUR
ALPHA_PULL = 0.05 * 2.0 * np.pi * 1000.0
KINDS = ("load300", "pull5", "pull5d")
CASES = [(n, k) for k in KINDS for n in FOUR] + [("beam", "beam")]


def beam_problem():
    mesh = meshgen.plate(32, 4, lx=1.0, ly=0.125)
    x = mesh.xy[:, 0]
    known = np.zeros((mesh.num_nodes, 2), dtype=np.uint8)
    known[x < x.min() + 1e-9] = 1
    f = np.zeros((mesh.num_nodes, 2))
    right = np.flatnonzero(x > x.max() - 1e-9)
    assert len(right) == 5
    f[right, 1] = -6e6 / 5
    return meshgen.Problem(mesh, known.reshape(-1), np.zeros(2 * mesh.num_nodes), f.reshape(-1))


@functools.lru_cache(maxsize=None)
def setup(name, kind):
    """dict(prob, M, m, free, K, steps, alpha, u0) with the lumped mass"""
    from test_load_cases_gpu import MESHES
    u0 = None
    if kind == "beam":
        prob, steps, alpha = beam_problem(), 1479, 0.0
    else:
        mesh = MESHES[name][0]().mesh
        steps = 256
        if kind == "load300":
            prob, alpha = meshgen.config_fixed_left_point_load(mesh, load=3e8), 0.0
        else:
            x = mesh.xy[:, 0]
            lx = x.max() - x.min()
            prob = meshgen.config_fixed_left_pull_right(mesh, delta=0.05 * lx)
            alpha = ALPHA_PULL if kind == "pull5d" else 0.0
            u0 = np.zeros((mesh.num_nodes, 2))
            u0[:, 0] = 0.05 * (x - x.min())
            u0 = u0.reshape(-1)
    K, M, free = modal_ref.matrices(prob, RHO, True)
    return dict(prob=prob, K=K, M=M, m=np.asarray(M.diagonal()), free=free, steps=steps, alpha=alpha, u0=u0)


@functools.lru_cache(maxsize=None)
def dt_of(name, kind):
    """0.9 of the twin's dt_bound (the device's own bound is used on the GPU: the two agree to 1e-14)"""
    s = setup(name, kind)
    return 0.9 * explicit_ref.bound(s["K"], s["m"], s["free"])


@functools.lru_cache(maxsize=None)
def twin(name, kind, dt):
    """the twin's run of the case at dt"""
    s = setup(name, kind)
    p = s["prob"]
    return ref.explicit_tl(p.mesh.xy, p.mesh.conn, p.youngs_modulus, p.poisson_ratio, p.part_thickness, s["M"], s["free"], p.u_in, p.f_in,
                           s["steps"], dt, s["alpha"], u0=s["u0"])


@functools.lru_cache(maxsize=None)
def linear(name, kind, dt):
    """the linear twin's run of the case at dt"""
    s = setup(name, kind)
    p = s["prob"]
    return explicit_ref.explicit(s["K"], s["M"], s["free"], p.u_in, p.f_in, s["steps"], dt, s["alpha"], 0.0, u0=s["u0"])


def force_of(prob, u):
    return ref.tl_force(prob.mesh.xy, prob.mesh.conn, prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness, u)


def rigid_motion(prob):
    """u of a rotation by 90 degrees about the centroid plus (0.3, -0.2)"""
    xy = prob.mesh.xy
    d = xy - xy.mean(axis=0)
    R = np.array([[0.0, -1.0], [1.0, 0.0]])
    return (d @ R.T - d + np.array([0.3, -0.2])).reshape(-1)
