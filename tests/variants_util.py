"""Design variants for the variant tests: morphed coordinates, drawn materials and load sets of ONE base problem (its
connectivity and u_known mask), and the stand-alone problem a variant amounts to."""
import dataclasses

import numpy as np

from load_cases_util import make_cases


def shortest_edge(xy, conn):
    p = xy[conn]
    return min(float(np.linalg.norm(p[:, a] - p[:, b], axis=1).min()) for a, b in ((0, 1), (1, 2), (2, 0)))


def signed_areas(xy, conn):
    p = xy.reshape(-1, 2)[conn]
    return 0.5 * (p[:, 0, 0] * (p[:, 1, 1] - p[:, 2, 1]) + p[:, 1, 0] * (p[:, 2, 1] - p[:, 0, 1]) + p[:, 2, 0] * (p[:, 0, 1] - p[:, 1, 1]))


def keeps_orientation(prob, xyv):
    a0, av = signed_areas(prob.mesh.xy, prob.mesh.conn), signed_areas(np.asarray(xyv), prob.mesh.conn)
    return bool(np.all(av != 0.0) and np.all((av > 0) == (a0 > 0)))


def morph(prob, a, k):
    """xy + a h (sin, cos) of a smooth field over the part, h the shortest edge, a <= 0.2: no element can turn over (a
    node moves by at most 0.2 h, an edge changes by at most 0.4 h).  k picks the field."""
    assert 0.0 <= a <= 0.2
    xy = prob.mesh.xy
    lo, span = xy.min(axis=0), np.ptp(xy, axis=0).max()
    s = (xy - lo) / span
    phase = 2.0 * np.pi * ((1 + k % 3) * s[:, 0] + (1 + (k // 3) % 3) * s[:, 1]) + 0.7 * k
    h = shortest_edge(xy, prob.mesh.conn)
    return (xy + a * h * np.stack([np.sin(phase), np.cos(phase)], axis=1)).reshape(-1)


def make_shapes(prob, V, amax=0.2):
    """(V, 2N): variant 0 keeps the uploaded shape, the others are morphs of growing amplitude and changing field."""
    xy = np.stack([morph(prob, amax * ((v % 7) / 6.0) if v else 0.0, v) for v in range(V)])
    for v in range(V):
        assert keeps_orientation(prob, xy[v]), v
    return xy


def make_materials(prob, V, seed=0):
    """(V, 3) = E in [0.5, 2] E0, nu in [0.2, 0.4], t in [0.5, 2] t0; variant 0: the problem's own material."""
    rng = np.random.default_rng(seed)
    m = np.stack([prob.youngs_modulus * rng.uniform(0.5, 2.0, V), rng.uniform(0.2, 0.4, V),
                  prob.part_thickness * rng.uniform(0.5, 2.0, V)], axis=1)
    m[0] = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
    return m


def make_variants(prob, V, seed=0):
    """Shape, material and loads all varied: xy (V, 2N), material (V, 3), u_in, f_in (V, 2N)."""
    u, f = make_cases(prob, V, seed=seed)
    return make_shapes(prob, V), make_materials(prob, V, seed), u, f


def variant_problem(prob, xy=None, material=None, u_in=None, f_in=None):
    """The problem variant (xy, material, u_in, f_in) is on its own (None: the base problem's)."""
    out = prob
    if xy is not None:
        out = dataclasses.replace(out, mesh=dataclasses.replace(out.mesh, xy=np.asarray(xy, dtype=np.float64).reshape(-1, 2).copy()))
    if material is not None:
        out = dataclasses.replace(out, youngs_modulus=float(material[0]), poisson_ratio=float(material[1]),
                                  part_thickness=float(material[2]))
    if u_in is not None:
        out = dataclasses.replace(out, u_in=np.ascontiguousarray(u_in), f_in=np.ascontiguousarray(f_in))
    return out
