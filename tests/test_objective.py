"""CPU: the reference of the objective tests gives the TOTAL derivative of both objectives -- explicit partials plus the adjoint
term against central differences of re-solved problems through the twin's direct solve, mixed boundary conditions --; its
stress is the twin's D B u_e; the entry points exist in header, binding and library, the structs have the header's layout, and
every argument and call-order error comes back before any HIP call, with its message."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import adjoint_ref as aref
import numpy_twin
import objective_ref as oref
import sensitivities_ref as sref
from magnetite_amd import _lib, meshgen
from test_adjoint import check, twin_u
from test_sensitivities import base_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
SYMBOLS = ("mag_run_objective", "mag_download_objective")


def test_reference_stress_is_the_twins_D_B_u():
    rng = np.random.default_rng(0)
    xy = rng.uniform(-1.0, 1.0, (30, 2))
    conn = np.array([rng.choice(30, 3, replace=False) for _ in range(40)], dtype=np.int32)
    area = np.array([numpy_twin.element_area(xy, t) for t in conn])
    assert (area > 0).any() and (area < 0).any()  # both orientations
    u = rng.standard_normal(60)
    sig = oref.element_stress(xy, conn, u, 0.31, 7e10)
    D = numpy_twin.stress_strain(0.31, 7e10)
    for e, tri in enumerate(conn):
        want = D @ numpy_twin.strain_displacement(xy, tri, area[e]) @ u.reshape(-1, 2)[tri].reshape(-1)
        assert np.abs(sig[e] - want).max() <= 1e-13 * np.abs(want).max(), e
    vm = np.sqrt(oref.von_mises_sq(sig))
    sx, sy, txy = sig.T
    assert np.allclose(vm, np.sqrt(0.5 * ((sx - sy) ** 2 + sx ** 2 + sy ** 2) + 3 * txy ** 2), rtol=1e-13)


def specs(prob, u):
    """kind -> the objective's arguments on the 120-node problem: a weighted p = 8 aggregate scaled by the largest von Mises
    stress of the base solution; a least-squares mismatch on a node patch against a target off the solution."""
    conn = np.asarray(prob.mesh.conn).reshape(-1, 3)
    sig = oref.element_stress(np.asarray(prob.mesh.xy).reshape(-1, 2), conn, u, prob.poisson_ratio, prob.youngs_modulus)
    scale = float(np.sqrt(oref.von_mises_sq(sig)).max())
    rng = np.random.default_rng(6)
    return {"stress_pnorm": dict(weights=rng.uniform(0.5, 1.5, len(conn)), p=8.0, scale=scale),
            "disp_lsq": dict(weights=aref.patch_weights(prob), target=0.7 * u + 0.1 * np.abs(u).max() * rng.standard_normal(u.size))}


@pytest.mark.parametrize("kind", ["stress_pnorm", "disp_lsq"])
def test_explicit_plus_adjoint_is_the_total_derivative_of_the_objective(kind):
    prob = base_problem(meshgen.config_fixed_left_pull_right)
    assert np.abs(prob.u_in[prob.u_known == 1]).max() > 0
    u = twin_u(prob)
    spec = specs(prob, u)[kind]
    got = oref.with_totals(kind, prob, u, **spec)
    assert got["J"] > 0
    if kind == "stress_pnorm":
        assert np.abs(got["pxy"]).max() > 0 and got["pJ_pt"] == 0.0
        assert abs(got["pJ_pE"] - got["J"] / prob.youngs_modulus) <= 1e-13 * got["J"] / prob.youngs_modulus
    else:
        assert not got["pxy"].any() and got["pJ_pE"] == got["pJ_pnu"] == got["pJ_pt"] == 0.0

    def J(p):
        return oref.of_problem(kind, p, twin_u(p), **spec)["J"]

    def central(vary, h):
        """fd at h and h / 2 of J over the problems vary(step)"""
        return [(J(vary(s)) - J(vary(-s))) / (2 * s) for s in (h, h / 2)]

    rng = np.random.default_rng(1)
    gmax = np.abs(got["dxy"]).max()
    assert gmax > 0
    for dof in rng.choice(got["dxy"].size, 12, replace=False):
        check(kind, ("dxy", dof), got["dxy"][dof], *central(lambda s: sref.moved(prob, dof, s), 1e-3 * 0.1), gmax)
    for key, field in (("dJ_dE", "youngs_modulus"), ("dJ_dnu", "poisson_ratio"), ("dJ_dt", "part_thickness")):
        v = getattr(prob, field)
        fd = central(lambda s: dataclasses.replace(prob, **{field: v + s}), 1e-3 * v)
        check(kind, key, got[key], *fd, abs(fd[1]))


def test_an_element_without_stress_contributes_nothing():
    xy = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=np.float64)
    conn = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    u = np.zeros(8)
    u[[6, 7]] = 1e-3, 2e-3  # node 3 moves: element 0 stays unstrained
    got = oref.stress_pnorm(xy, conn, u, 7e10, 0.3, 0.01, p=1.5, scale=1e8)
    assert got["J"] > 0 and np.isfinite(got["g"]).all() and np.isfinite(got["pxy"]).all()
    assert not got["g"][[0, 1]].any() and not got["pxy"][[0, 1]].any()  # node 0 belongs to element 0 only
    none = oref.stress_pnorm(xy, conn, np.zeros(8), 7e10, 0.3, 0.01, p=8.0, scale=1e8)
    assert none["J"] == 0.0 and not none["g"].any() and not none["pxy"].any()


def test_struct_layout_symbols_and_header(built):
    assert C.sizeof(_lib.Objective) == 48 and C.sizeof(_lib.ObjectiveResult) == 96
    offsets = {name: getattr(_lib.Objective, name).offset for name, _ in _lib.Objective._fields_}
    assert offsets == dict(kind=0, per_member=4, p=8, scale=16, weights=24, target=32, memory=40, reserved=44)
    offsets = {name: getattr(_lib.ObjectiveResult, name).offset for name, _ in _lib.ObjectiveResult._fields_}
    assert offsets == dict(g_out=0, pxy_out=8, dxy_out=16, scalars=24, memory=88, reserved=92)
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4 and "MAG_ABI_VERSION 4" in header
    assert "enum mag_objective_kind { MAG_OBJ_DISP_LSQ = 0, MAG_OBJ_STRESS_PNORM = 1 }" in header
    assert (_lib.MAG_OBJ_DISP_LSQ, _lib.MAG_OBJ_STRESS_PNORM) == (0, 1)
    assert "} mag_objective;" in header and "} mag_objective_result;" in header


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        w = (C.c_double * 4)()
        wp = C.cast(w, C.c_void_p).value

        def lsq(**kw):
            return _lib.Objective(**{**dict(kind=_lib.MAG_OBJ_DISP_LSQ, weights=wp), **kw})

        def pnorm(**kw):
            return _lib.Objective(**{**dict(kind=_lib.MAG_OBJ_STRESS_PNORM, p=8.0, scale=1.0), **kw})

        def run(s, o, adjoint=0):
            return L.mag_run_objective(h, s, C.byref(o) if o is not None else None, adjoint)

        out = _lib.ObjectiveResult()
        assert L.mag_run_objective(None, 0, C.byref(lsq()), 0) == MAG_ERR_BAD_ARGS
        assert L.mag_download_objective(None, 0, 0, C.byref(out)) == MAG_ERR_BAD_ARGS
        for bad in (-1, 3, 99):
            assert run(bad, lsq()) == MAG_ERR_BAD_ARGS
            assert b"mag_set" in L.mag_last_error(h)
            assert L.mag_download_objective(h, bad, 0, C.byref(out)) == MAG_ERR_BAD_ARGS
            assert b"mag_set" in L.mag_last_error(h)
        for s, fn in ((0, b"mag_run"), (1, b"mag_run_cases"), (2, b"mag_run_variants")):
            for adjoint in (0, 1):
                assert run(s, None, adjoint) == MAG_ERR_BAD_ARGS
                assert b"null objective" in L.mag_last_error(h)
                for kind in (-1, 2, 7):
                    assert run(s, lsq(kind=kind), adjoint) == MAG_ERR_BAD_ARGS
                    assert b"mag_objective_kind" in L.mag_last_error(h)
                assert run(s, lsq(weights=None), adjoint) == MAG_ERR_BAD_ARGS
                assert b"weights" in L.mag_last_error(h)
                for p in (0.999, 0.0, -2.0, float("nan"), float("inf")):
                    assert run(s, pnorm(p=p), adjoint) == MAG_ERR_BAD_ARGS, p
                    assert b"p = " in L.mag_last_error(h)
                for scale in (0.0, -1.0, float("nan"), float("inf")):
                    assert run(s, pnorm(scale=scale), adjoint) == MAG_ERR_BAD_ARGS, scale
                    assert b"scale = " in L.mag_last_error(h)
                # no completed run of that set: both kinds, null weights allowed for the p-norm
                for o in (lsq(), pnorm(), pnorm(weights=wp), pnorm(p=1.0)):
                    assert run(s, o, adjoint) == MAG_ERR_STATE
                    assert b"mag_run_objective before a completed " + fn in L.mag_last_error(h)
            assert L.mag_download_objective(h, s, 0, None) == MAG_ERR_BAD_ARGS
            assert b"null objective result" in L.mag_last_error(h)
            assert L.mag_download_objective(h, s, -1, C.byref(out)) == MAG_ERR_BAD_ARGS
            assert b"out of range" in L.mag_last_error(h)
            assert L.mag_download_objective(h, s, 0, C.byref(out)) == MAG_ERR_STATE
            assert fn in L.mag_last_error(h)
        # a communicator of more than one rank
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        for s in (0, 1, 2):
            assert run(s, lsq()) == MAG_ERR_BAD_ARGS
            assert b"communicator" in L.mag_last_error(h)
            assert run(s, pnorm(), 1) == MAG_ERR_BAD_ARGS
            assert L.mag_download_objective(h, s, 0, C.byref(out)) == MAG_ERR_BAD_ARGS
            assert b"communicator" in L.mag_last_error(h)
    finally:
        L.mag_destroy(h)


def test_python_mirror_names_sets_and_kinds(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        with pytest.raises(MagnetiteError):
            c.objective("disp_lsq", "all", weights=np.zeros(4))
        with pytest.raises(MagnetiteError):
            c.objective("compliance", weights=np.zeros(4))
        with pytest.raises(MagnetiteError):
            c.objective("disp_lsq", weights=np.zeros(4), target=np.zeros((1, 4)))  # one row and a row per member
        for s in ("run", "cases", "variants"):
            for kind, kw in (("disp_lsq", dict(weights=np.zeros(4))), ("stress_pnorm", {})):
                with pytest.raises(MagnetiteError) as e:
                    c.objective(kind, s, **kw)
                assert e.value.code == MAG_ERR_STATE
            with pytest.raises(MagnetiteError) as e:
                c.download_objective(s, 0)
            assert e.value.code == MAG_ERR_STATE
