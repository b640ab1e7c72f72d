"""The cases of the explicit-dynamics tests (CPU and GPU): the four meshes of tests/test_load_cases_gpu.py as uploaded ("pull")
and under config_fixed_left_point_load ("load"), one plate(4) on rollers, the project's damped set; everything computed once,
shared, left unchanged."""
import functools

import numpy as np

import explicit_ref as ref
import modal_ref
from magnetite_amd import meshgen

RHO = 2700.0
FOUR = ("plate16", "holes3k", "frontal3k", "two_fans")


def rollers():
    """plate(4): x fixed on the left edge, y at one node (the lower left corner), a point load on the right edge"""
    mesh = meshgen.plate(4)
    prob = meshgen.config_fixed_left_point_load(mesh)
    x, y = mesh.xy[:, 0], mesh.xy[:, 1]
    known = np.zeros((mesh.num_nodes, 2), dtype=np.uint8)
    known[x < x.min() + 1e-9, 0] = 1
    known[int(np.argmin(x + y)), 1] = 1
    return meshgen.Problem(mesh, known.reshape(-1), np.zeros(2 * mesh.num_nodes), np.array(prob.f_in, dtype=np.float64).reshape(-1))


@functools.lru_cache(maxsize=None)
def setup(name, config):
    """(prob, K, M, m, free, omega_1, T1) with the lumped mass"""
    from test_load_cases_gpu import MESHES
    if name == "rollers":
        prob = rollers()
    else:
        prob = MESHES[name][0]()
        if config == "load":
            prob = meshgen.config_fixed_left_point_load(prob.mesh)
    K, M, free = modal_ref.matrices(prob, RHO, True)
    lam, _ = modal_ref.eigenpairs(K, M, free, 2)
    w1 = float(np.sqrt(lam[0]))
    return prob, K, M, np.asarray(M.diagonal()), free, w1, 2.0 * np.pi / w1


def rayleigh(which, w1):
    """(alpha, eta): undamped, or the project's damped set"""
    return (0.0, 0.0) if which == "undamped" else (0.05 * w1, 0.02 / w1)


def amplitude_of(config, dt, T1, steps):
    return 1.0 + np.sin(2.0 * np.pi * np.arange(steps + 1) * dt / (0.7 * T1)) if config == "load" else None


@functools.lru_cache(maxsize=None)
def omega_max(name, config):
    prob, K, M, m, free, w1, T1 = setup(name, config)
    return ref.omega_max(K, m, free)


CASES = [(n, c) for n in FOUR for c in ("pull", "load")] + [("rollers", "load")]
