"""CPU: the reference of the sensitivity tests restates the reference's K_e; 1/2 u^T (dK/dtheta) u IS the total derivative of the
potential energy (finite differences of re-solved problems, mixed boundary conditions); the entry points exist in header,
binding and library and their argument and call-order errors come back before any HIP call."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import numpy_twin
import sensitivities_ref as ref
from magnetite_amd import _lib, meshgen
from variants_util import morph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7


def test_reference_energy_equals_the_twins_element_stiffness():
    rng = np.random.default_rng(0)
    xy = rng.uniform(-1.0, 1.0, (30, 2))
    conn = np.array([rng.choice(30, 3, replace=False) for _ in range(40)], dtype=np.int32)
    area = np.array([numpy_twin.element_area(xy, t) for t in conn])
    assert (area > 0).any() and (area < 0).any()  # both orientations
    u = rng.standard_normal(60)
    K = ref.element_stiffness(xy, conn, 0.31, 7e10, 0.02)
    energy = ref.element_energy(xy, conn, u, 0.31, 7e10, 0.02)
    for e, tri in enumerate(conn):
        Ke = numpy_twin.element_stiffness(xy, tri, 0.31, 7e10, 0.02)
        assert np.abs(K[e] - Ke).max() <= 1e-13 * np.abs(Ke).max(), e
        ue = u.reshape(-1, 2)[tri].reshape(-1)
        want = 0.5 * ue @ Ke @ ue
        assert abs(energy[e] - want) <= 1e-12 * np.abs(Ke).max() * (ue @ ue), e
        assert (energy[e] > 0) == (area[e] > 0)  # the signed area's sign


def base_problem(config):
    mesh = meshgen.shuffle(meshgen.plate_with_holes(10), 3)
    assert mesh.num_nodes == 120
    prob = config(mesh)
    xy = morph(prob, 0.15, 4).reshape(-1, 2)
    prob = dataclasses.replace(prob, mesh=dataclasses.replace(prob.mesh, xy=xy))
    if config is meshgen.config_fixed_left_pull_right:  # mixed: prescribed displacements AND forces on the free DOFs
        rng = np.random.default_rng(5)
        free = prob.u_known == 0
        k_scale = prob.youngs_modulus * prob.part_thickness * prob.meta["delta"]
        prob = dataclasses.replace(prob, f_in=np.where(free, 0.05 * k_scale * rng.standard_normal(free.size), 0.0))
    return prob


@pytest.mark.parametrize("config", [meshgen.config_fixed_left_pull_right, meshgen.config_fixed_left_point_load])
def test_the_gradient_is_the_total_derivative_of_the_potential(config):
    prob = base_problem(config)
    sol = ref.direct_solution(prob)
    got = ref.of_solution(prob, sol)
    g = got["dxy"]
    gmax = np.abs(g).max()
    assert abs(got["potential_energy"] - ref.potential(prob)) <= 1e-12 * abs(got["strain_energy"])
    h = 1e-3 * 0.1  # of the cell pitch
    rng = np.random.default_rng(1)
    for dof in rng.choice(g.size, 12, replace=False):
        fd = [(ref.potential(ref.moved(prob, dof, s)) - ref.potential(ref.moved(prob, dof, -s))) / (2 * s) for s in (h, h / 2)]
        err, rich = abs(g[dof] - fd[1]), abs(fd[0] - fd[1])
        print(config.__name__, "dof", dof, "g", g[dof], "err/max|g|", err / gmax, "richardson/max|g|", rich / gmax)
        assert err <= 4 * rich + 2e-7 * gmax, dof
    # E, nu, t: central differences at a relative step of 1e-5, to 1e-8 of the quotient
    for key, field in (("dPi_dE", "youngs_modulus"), ("dPi_dnu", "poisson_ratio"), ("dPi_dt", "part_thickness")):
        v = getattr(prob, field)
        fd = (ref.potential(dataclasses.replace(prob, **{field: v * (1 + 1e-5)})) -
              ref.potential(dataclasses.replace(prob, **{field: v * (1 - 1e-5)}))) / (2e-5 * v)
        print(config.__name__, key, got[key], "rel", abs(got[key] - fd) / abs(fd))
        assert abs(got[key] - fd) <= 1e-8 * abs(fd), key
    # translation invariance: the sum over all nodes is zero to 1e-15 of max|g| (on the reference's unrounded entries)
    assert np.abs(got["dxy_ext"] - g).max() <= np.finfo(np.float64).eps * gmax
    for d in (0, 1):
        total = abs(np.sum(got["dxy_ext"][d::2]))
        print(config.__name__, "sum of dxy, axis", d, "of max|g|", float(total / gmax))
        assert total <= 1e-15 * gmax, d


def test_struct_size_symbols_and_header(built):
    assert C.sizeof(_lib.Sensitivity) == 88
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    L = _lib.lib()
    for name in ("mag_run_sensitivities", "mag_download_sensitivity"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4 and "MAG_ABI_VERSION 4" in header
    assert "enum mag_set { MAG_SET_RUN = 0, MAG_SET_CASES = 1, MAG_SET_VARIANTS = 2 }" in header
    assert (_lib.MAG_SET_RUN, _lib.MAG_SET_CASES, _lib.MAG_SET_VARIANTS) == (0, 1, 2)


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        o = _lib.Sensitivity()
        assert L.mag_run_sensitivities(None, 0) == MAG_ERR_BAD_ARGS
        for bad in (-1, 3, 99):
            assert L.mag_run_sensitivities(h, bad) == MAG_ERR_BAD_ARGS
            assert b"mag_set" in L.mag_last_error(h)
            assert L.mag_download_sensitivity(h, bad, 0, C.byref(o)) == MAG_ERR_BAD_ARGS
        assert L.mag_download_sensitivity(None, 0, 0, C.byref(o)) == MAG_ERR_BAD_ARGS
        assert L.mag_download_sensitivity(h, 0, 0, None) == MAG_ERR_BAD_ARGS
        assert L.mag_download_sensitivity(h, 0, -1, C.byref(o)) == MAG_ERR_BAD_ARGS
        for s, fn in ((0, b"mag_run"), (1, b"mag_run_cases"), (2, b"mag_run_variants")):
            assert L.mag_run_sensitivities(h, s) == MAG_ERR_STATE  # no completed run of that set
            assert fn in L.mag_last_error(h)
            assert L.mag_download_sensitivity(h, s, 0, C.byref(o)) == MAG_ERR_STATE
    finally:
        L.mag_destroy(h)


def test_python_mirror_names_the_sets(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        with pytest.raises(MagnetiteError):
            c.sensitivities("all")
        for s in ("run", "cases", "variants"):
            with pytest.raises(MagnetiteError) as e:
                c.sensitivities(s)
            assert e.value.code == MAG_ERR_STATE
