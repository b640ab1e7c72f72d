"""Load sets for the load-case tests: one u_known mask (the base problem's), other prescribed values per case."""
import dataclasses

import numpy as np


def make_cases(prob, num_cases, seed=0, force_scale=None):
    """(L, 2N) arrays u_in, f_in.  Case 0: the problem's own loads; case 1: 1e-3 x case 0 (another iteration count under
    the absolute stop rule); the others: the prescribed displacements and forces scaled, plus seeded random nodal forces
    on the free DOFs."""
    rng = np.random.default_rng(seed)
    free = prob.u_known == 0
    if force_scale is None:  # forces of the size the base problem's own loads produce (or its point load)
        force_scale = max(float(np.abs(prob.f_in).max()), 1e3)
    scales = (1.0, 1e-3, 0.5, 2.0, -1.0, 0.25, 3.0, -0.5)
    u = np.empty((num_cases, prob.u_in.size))
    f = np.empty((num_cases, prob.f_in.size))
    for c in range(num_cases):
        s = scales[c % len(scales)] * (1.0 + 0.01 * (c // len(scales)))
        u[c] = np.where(free, 0.0, prob.u_in * s)
        f[c] = np.where(free, prob.f_in * s, 0.0)
        if c >= 2:
            f[c] += np.where(free, rng.standard_normal(prob.f_in.size) * force_scale * 1e-2, 0.0)
    return u, f


def case_problem(prob, u_in, f_in):
    return dataclasses.replace(prob, u_in=np.ascontiguousarray(u_in), f_in=np.ascontiguousarray(f_in))


def patch_mesh(nx=12, ny=6, L=2.0, H=1.0):
    """The mesh of tests/cpp/run_patch.cpp / run_cases.cpp, node for node: xy (N, 2), conn (E, 3)."""
    xy = np.array([[L * i / nx, H * j / ny] for j in range(ny + 1) for i in range(nx + 1)])
    conn = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            b, c = a + 1, a + nx + 1
            d = c + 1
            conn += [[a, b, d], [a, d, c]]
    return xy, np.array(conn, dtype=np.int32)


def patch_cases(nx=12, ny=6):
    """The two load sets of tests/cpp/run_cases.cpp: u_known (2N,), u_in (2, 2N), f_in (2, 2N)."""
    N = (nx + 1) * (ny + 1)
    delta, pull = (1e-3, 2.5e-4), (0.0, 1.0e4)
    known = np.zeros((N, 2), dtype=np.uint8)
    u = np.zeros((2, N, 2))
    f = np.zeros((2, N, 2))
    for j in range(ny + 1):
        for i in range(nx + 1):
            n = j * (nx + 1) + i
            if i == 0:
                known[n, 0] = 1
                if j == 0:
                    known[n, 1] = 1
            if i == nx:
                known[n, 0] = 1
                u[:, n, 0] = delta
            if j == ny and 0 < i < nx:
                f[:, n, 1] = pull
    return known.reshape(-1), u.reshape(2, -1), f.reshape(2, -1)
