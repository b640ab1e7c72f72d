"""CPU: the reference of the adjoint tests IS the total derivative of an objective -- central differences of re-solved problems
through the twin's direct solve, mixed boundary conditions with nonzero prescribed displacements, two objectives --; where the
problem is self-adjoint it reduces to the energy sensitivities; the entry points exist in header, binding and library and their
argument and call-order errors come back before any HIP call."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import adjoint_ref as aref
import numpy_twin
import sensitivities_ref as sref
from magnetite_amd import _lib, meshgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
SYMBOLS = ("mag_run_adjoint", "mag_download_adjoint", "mag_get_adjoint_stats", "mag_get_adjoint_info")


def mixed_problem():
    """plate(8): left edge fixed, right edge pulled by a NONZERO prescribed displacement, seeded forces on the free DOFs."""
    prob = meshgen.config_fixed_left_pull_right(meshgen.plate(8))
    free = prob.u_known == 0
    k_scale = prob.youngs_modulus * prob.part_thickness * prob.meta["delta"]
    f_in = np.where(free, 0.05 * k_scale * np.random.default_rng(5).standard_normal(free.size), 0.0)
    return dataclasses.replace(prob, f_in=f_in)


def twin_u(prob, scale=None):
    """u of the twin's direct solve; with `scale` (E,), of the problem whose K is the sum of scale[e] K_e."""
    xy, conn = prob.mesh.xy, prob.mesh.conn
    mat = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
    if scale is None:
        return numpy_twin.solve(xy, conn, prob.u_known, prob.u_in, prob.f_in, *mat)["u"]
    K = np.zeros((2 * len(xy), 2 * len(xy)))
    for e, tri in enumerate(conn):
        dofs = np.array([[2 * i, 2 * i + 1] for i in tri]).reshape(-1)
        K[np.ix_(dofs, dofs)] += scale[e] * numpy_twin.element_stiffness(xy, tri, mat[1], mat[0], mat[2])
    free, known = np.where(prob.u_known == 0)[0], np.where(prob.u_known == 1)[0]
    u = np.array(prob.u_in, dtype=np.float64)
    u[free] = np.linalg.solve(K[np.ix_(free, free)], prob.f_in[free] - K[np.ix_(free, known)] @ prob.u_in[known])
    return u


def objectives(prob):
    """name -> (J(u), dJ/du(u)): J1 = sum w u^2 over a node patch, J2 = c^T u with c on free AND prescribed DOFs."""
    w = aref.patch_weights(prob)
    rng = np.random.default_rng(9)
    c = np.zeros(prob.u_known.size)
    free, known = np.where(prob.u_known == 0)[0], np.where(prob.u_known == 1)[0]
    c[rng.choice(free, 10, replace=False)] = rng.standard_normal(10)
    c[rng.choice(known, 8, replace=False)] = rng.standard_normal(8)
    return {"J1": (lambda u: aref.J1(w, u), lambda u: aref.dJ1(w, u)), "J2": (lambda u: float(c @ u), lambda u: c.copy())}


def check(name, what, got, fd_h, fd_h2, gmax):
    err, rich = abs(got - fd_h2), abs(fd_h - fd_h2)
    print(name, what, "got", got, "fd", fd_h2, "err/max|g|", err / gmax, "richardson/max|g|", rich / gmax)
    assert err <= 4 * rich + 2e-7 * gmax, (name, what)


@pytest.mark.parametrize("name", ["J1", "J2"])
def test_the_adjoint_formula_is_the_total_derivative_of_the_objective(name):
    prob = mixed_problem()
    assert np.abs(prob.u_in[prob.u_known == 1]).max() > 0
    J, dJ = objectives(prob)[name]
    u = twin_u(prob)
    g = dJ(u)
    got = aref.of_problem(prob, u, g)
    rng = np.random.default_rng(1)

    def central(vary, h):
        """fd at h and h / 2 of J over the problems vary(step)"""
        return [(J(twin_u(*vary(s))) - J(twin_u(*vary(-s)))) / (2 * s) for s in (h, h / 2)]

    # 12 random coordinates
    gmax = np.abs(got["dxy"]).max()
    assert gmax > 0
    for dof in rng.choice(got["dxy"].size, 12, replace=False):
        check(name, ("dxy", dof), got["dxy"][dof], *central(lambda s: (sref.moved(prob, dof, s),), 1e-3 / 8), gmax)
    # E, nu, t
    for key, field in (("dJ_dE", "youngs_modulus"), ("dJ_dnu", "poisson_ratio"), ("dJ_dt", "part_thickness")):
        v = getattr(prob, field)
        fd = central(lambda s: (dataclasses.replace(prob, **{field: v + s}),), 1e-3 * v)
        check(name, key, got[key], *fd, abs(fd[1]))
    # the loads: 6 free DOFs (forces), 6 prescribed ones (displacements; J2's c reaches some of them)
    free, known = np.where(prob.u_known == 0)[0], np.where(prob.u_known == 1)[0]

    def loaded(field, dof, s):
        v = getattr(prob, field).copy()
        v[dof] += s
        return (dataclasses.replace(prob, **{field: v}),)

    picks_known = rng.choice(known, 6, replace=False)
    if name == "J2":
        picks_known[:3] = known[g[known] != 0][:3]
    for field, dofs, h in (("f_in", rng.choice(free, 6, replace=False), 1e-3 * np.abs(prob.f_in).max()),
                           ("u_in", picks_known, 1e-3 * prob.meta["delta"])):
        gmax = np.abs(got["dloads"][free if field == "f_in" else known]).max()
        for dof in dofs:
            check(name, (field, dof), got["dloads"][dof], *central(lambda s: loaded(field, dof, s), h), gmax)
    # a relative stiffness scale per element
    E = len(prob.mesh.conn)
    gmax = np.abs(got["delem"]).max()

    def scaled(e, s):
        scale = np.ones(E)
        scale[e] += s
        return prob, scale

    for e in rng.choice(E, 6, replace=False):
        check(name, ("delem", e), got["delem"][e], *central(lambda s: scaled(e, s), 1e-3), gmax)


def test_self_adjoint_case_reduces_to_the_energy_sensitivities():
    """Prescribed displacements all zero and g = f_in on the free DOFs: lambda = u, dxy = -2 x the energy gradient,
    delem = -2 x the element energies, a = 2 W."""
    prob = meshgen.config_fixed_left_point_load(meshgen.shuffle(meshgen.plate_with_holes(10), 3))
    free = prob.u_known == 0
    f_in = np.where(free, prob.f_in + 1e4 * np.random.default_rng(3).standard_normal(free.size), 0.0)
    prob = dataclasses.replace(prob, f_in=f_in)
    assert not prob.u_in.any()
    sol = sref.direct_solution(prob)
    g = np.where(free, prob.f_in, 0.0)
    got = aref.of_problem(prob, sol["u"], g)
    want = sref.of_solution(prob, sol)
    assert np.abs(got["lambda"] - sol["u"]).max() <= 1e-12 * np.abs(sol["u"]).max()
    # (lambda is a second solve of the same system: compare the formulas on the SAME vector)
    mat = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
    same = aref.adjoint(prob.mesh.xy, prob.mesh.conn, prob.u_known, sol["u"], sol["u"], g, sol["f"], *mat)
    assert np.abs(same["dxy"] + 2 * want["dxy"]).max() <= 1e-12 * np.abs(want["dxy"]).max()
    assert np.abs(same["delem"] + 2 * want["energy"]).max() <= 1e-12 * np.abs(want["energy"]).max()
    assert abs(same["a"] - 2 * want["strain_energy"]) <= 1e-12 * abs(want["strain_energy"])
    assert abs(same["dJ_dnu"] + 2 * want["dPi_dnu"]) <= 1e-12 * abs(want["dPi_dnu"])
    assert np.array_equal(same["dloads"][free], sol["u"][free])


def test_struct_size_symbols_and_header(built):
    assert C.sizeof(_lib.Adjoint) == 104
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4 and "MAG_ABI_VERSION 4" in header
    assert "} mag_adjoint;" in header


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        o, st, info = _lib.Adjoint(), _lib.Stats(), (C.c_int32 * 4)()
        g = (C.c_double * 4)()
        assert L.mag_run_adjoint(None, 0, g, 0) == MAG_ERR_BAD_ARGS
        assert L.mag_download_adjoint(None, 0, 0, C.byref(o)) == MAG_ERR_BAD_ARGS
        assert L.mag_get_adjoint_stats(None, 0, 0, C.byref(st)) == MAG_ERR_BAD_ARGS
        assert L.mag_get_adjoint_info(None, 0, info) == MAG_ERR_BAD_ARGS
        for bad in (-1, 3, 99):
            assert L.mag_run_adjoint(h, bad, g, 0) == MAG_ERR_BAD_ARGS
            assert b"mag_set" in L.mag_last_error(h)
            assert L.mag_download_adjoint(h, bad, 0, C.byref(o)) == MAG_ERR_BAD_ARGS
            assert L.mag_get_adjoint_stats(h, bad, 0, C.byref(st)) == MAG_ERR_BAD_ARGS
            assert L.mag_get_adjoint_info(h, bad, info) == MAG_ERR_BAD_ARGS
        for s, fn in ((0, b"mag_run"), (1, b"mag_run_cases"), (2, b"mag_run_variants")):
            assert L.mag_run_adjoint(h, s, None, 0) == MAG_ERR_BAD_ARGS  # null dJ_du
            assert L.mag_download_adjoint(h, s, 0, None) == MAG_ERR_BAD_ARGS  # null out
            assert L.mag_get_adjoint_stats(h, s, 0, None) == MAG_ERR_BAD_ARGS
            assert L.mag_get_adjoint_info(h, s, None) == MAG_ERR_BAD_ARGS
            assert L.mag_download_adjoint(h, s, -1, C.byref(o)) == MAG_ERR_BAD_ARGS  # index out of range
            assert L.mag_get_adjoint_stats(h, s, -1, C.byref(st)) == MAG_ERR_BAD_ARGS
            assert L.mag_run_adjoint(h, s, g, 0) == MAG_ERR_STATE  # no completed run of that set
            assert fn in L.mag_last_error(h)
            assert L.mag_download_adjoint(h, s, 0, C.byref(o)) == MAG_ERR_STATE  # ... and no mag_run_adjoint of it
            assert L.mag_get_adjoint_stats(h, s, 0, C.byref(st)) == MAG_ERR_STATE
            assert L.mag_get_adjoint_info(h, s, info) == MAG_ERR_STATE
        # a communicator of more than one rank
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        for s in (0, 1, 2):
            assert L.mag_run_adjoint(h, s, g, 0) == MAG_ERR_BAD_ARGS
            assert b"communicator" in L.mag_last_error(h)
            assert L.mag_download_adjoint(h, s, 0, C.byref(o)) == MAG_ERR_BAD_ARGS
            assert L.mag_get_adjoint_stats(h, s, 0, C.byref(st)) == MAG_ERR_BAD_ARGS
            assert L.mag_get_adjoint_info(h, s, info) == MAG_ERR_BAD_ARGS
    finally:
        L.mag_destroy(h)


def test_python_mirror_names_the_sets(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        with pytest.raises(MagnetiteError):
            c.adjoint(np.zeros((1, 4)), "all")
        with pytest.raises(MagnetiteError):
            c.adjoint(np.zeros(4), "cases")  # one row per member
        for s in ("run", "cases", "variants"):
            with pytest.raises(MagnetiteError) as e:
                c.adjoint(np.zeros((1, 4)), s)
            assert e.value.code == MAG_ERR_STATE
            for getter in (lambda: c.download_adjoint(s, 0), lambda: c.adjoint_stats(s, 0), lambda: c.adjoint_info(s)):
                with pytest.raises(MagnetiteError) as e:
                    getter()
                assert e.value.code == MAG_ERR_STATE
