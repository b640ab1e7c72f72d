"""No GPU: the numpy twin of the total-Lagrangian internal force (tests/explicit_tl_ref.py) -- its linearisation is K, a rigid
motion gives no force, its energy is the sum of A t S:E / 2 and its force the gradient of that energy; the cases are what
tests/explicit_tl_cases.py says; the ABI of kinematics and mag_internal_force (struct layout against a compiled offsetof,
symbols, defaults), every refusal that precedes any HIP call and the Python mirror's argument check.

Bars (from the issue) and what was measured:
  rel(tl_force(eps w), eps K w) <= 100 eps on plate16: 3.9e-2, 3.8e-4, 3.8e-6 at eps = 1e-3, 1e-5, 1e-7;
  |tl_force(rigid motion)| <= 1e-12 |K u|: 9.6e-16;
  W against the independent sum: 1e-13 relative, a sum of 512 terms of one sign (8.9e-16);
  a central difference of W in 8 random DOFs against f_int there: 1e-6 relative (3.8e-9)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import explicit_tl_cases as cases
import explicit_tl_ref as ref
from magnetite_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
RHO = cases.RHO


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def plate16():
    s = cases.setup("plate16", "load300")
    return s["prob"], s["K"]


def test_the_linearisation_at_zero_is_k():
    prob, K = plate16()
    w = np.random.default_rng(0).standard_normal(K.shape[0])
    for eps in (1e-3, 1e-5, 1e-7):
        f, W, det = cases.force_of(prob, eps * w)
        err = rel(f, eps * (K @ w))
        print("eps", eps, "rel(tl_force(eps w), eps K w)", err)
        assert err <= 100 * eps


def test_a_rigid_motion_gives_no_force():
    prob, K = plate16()
    u = cases.rigid_motion(prob)
    f, W, det = cases.force_of(prob, u)
    share = np.linalg.norm(f) / np.linalg.norm(K @ u)
    print("|tl_force(u)| / |K u|", share, "W", W, "det F", det)
    assert share <= 1e-12 and abs(det - 1.0) <= 1e-12


def moved(prob, K, scale=2e-2, seed=3):
    """a state with strains of a few percent: the linear static answer's shape is of no interest, any smooth large u does"""
    xy = prob.mesh.xy
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((2, 6))
    x, y = xy[:, 0], xy[:, 1]
    basis = np.stack([x, y, x * y, x * x, y * y, np.sin(3 * x + 2 * y)], axis=0)
    return scale * (c @ basis).T.reshape(-1)


def test_the_energy_is_the_sum_of_the_elements_energies():
    prob, K = plate16()
    u = moved(prob, K)
    f, W, det = cases.force_of(prob, u)
    # independently: E = (F^T F - I) / 2 from the deformed edges, S = D E in Voigt form, W_e = A t S:E / 2
    xy, conn = prob.mesh.xy, prob.mesh.conn
    E_, nu, t = prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness
    D = E_ / (1 - nu * nu) * np.array([[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]])
    x = xy + u.reshape(-1, 2)
    total = 0.0
    for a, b, c in conn:
        X0 = np.column_stack([xy[b] - xy[a], xy[c] - xy[a]])
        X1 = np.column_stack([x[b] - x[a], x[c] - x[a]])
        F = X1 @ np.linalg.inv(X0)
        G = 0.5 * (F.T @ F - np.eye(2))
        e = np.array([G[0, 0], G[1, 1], 2 * G[0, 1]])
        total += 0.5 * np.linalg.det(X0) * t * (e @ D @ e) / 2
    print("W", W, "the independent sum", total, abs(W - total) / total)
    assert 0.8 < det < 1.2 and abs(W - total) <= 1e-13 * total


def test_the_force_is_the_gradient_of_the_energy():
    prob, K = plate16()
    u = moved(prob, K)
    f, W, det = cases.force_of(prob, u)
    dofs = np.random.default_rng(5).choice(u.size, 8, replace=False)
    h = 1e-6
    fd = np.empty(8)
    for k, d in enumerate(dofs):
        up, um = u.copy(), u.copy()
        up[d] += h
        um[d] -= h
        fd[k] = (cases.force_of(prob, up)[1] - cases.force_of(prob, um)[1]) / (2 * h)
    print("central difference of W against f_int", rel(fd, f[dofs]), fd, f[dofs])
    assert rel(fd, f[dofs]) <= 1e-6


@pytest.mark.parametrize("name, kind", [("plate16", "load300"), ("plate16", "pull5"), ("plate16", "pull5d"), ("beam", "beam")])
def test_the_cases_are_finite_uninverted_and_far_from_linear(name, kind):
    dt = cases.dt_of(name, kind)
    tl, lin = cases.twin(name, kind, dt), cases.linear(name, kind, dt)
    apart = float(rel(tl["u"][-1], lin["u"][-1]))
    print(name, kind, "min det F", tl["min_det"], "TL and linear apart by", apart, "max |u|", np.abs(tl["u"][-1]).max())
    assert np.isfinite(tl["u"]).all() and np.isfinite(tl["a"]).all()
    assert 0.83 <= tl["min_det"] <= 1.01
    assert apart >= 8e-3


def test_struct_layout_symbols_and_defaults(built, tmp_path):
    cname, cls = "mag_explicit_options", _lib.ExplicitOptions
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "magnetite_hip.h"', "int main(void){",
             f'printf("{cname} %zu\\n", sizeof({cname}));', f'printf("kin %d %d\\n", MAG_KIN_LINEAR, MAG_KIN_TOTAL_LAGRANGIAN);']
    for f, _ in cls._fields_:
        lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 104
    assert got["kin"].split() == ["0", "1"] and (_lib.MAG_KIN_LINEAR, _lib.MAG_KIN_TOTAL_LAGRANGIAN) == (0, 1)
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    assert cls.kinematics.offset == 28 and cls.kinematics.size == 4
    assert "reserved" not in dict(cls._fields_)
    L = _lib.lib()
    assert L.mag_version() == 4
    assert "mag_internal_force" in _lib.SYMBOLS and L.mag_internal_force.argtypes is not None
    o = _lib.ExplicitOptions(steps=9, kinematics=1)
    L.mag_default_explicit_options(C.byref(o))
    assert o.kinematics == 0
    from magnetite_amd import Context
    assert callable(Context.internal_force) and Context.KINEMATICS == dict(linear=0, tl=1)


def test_refusals_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    x, f, sc = np.zeros(8), np.zeros(8), np.zeros(2)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    try:
        def opts(**kw):
            o = _lib.ExplicitOptions()
            L.mag_default_explicit_options(C.byref(o))
            for k, v in {**dict(steps=4, density=RHO), **kw}.items():
                setattr(o, k, v)
            return o

        def refused(rc, code, *words):
            msg = L.mag_last_error(h)
            assert rc == code, (rc, msg)
            for w in words:
                assert w in msg, (w, msg)

        for kin in (2, -1, 7):
            refused(L.mag_run_explicit(h, C.byref(opts(kinematics=kin))), MAG_ERR_BAD_ARGS, b"mag_run_explicit", b"kinematics", str(kin).encode())
        refused(L.mag_run_explicit(h, C.byref(opts(kinematics=1, rayleigh_stiffness=1e-7))), MAG_ERR_BAD_ARGS, b"mag_run_explicit",
                b"rayleigh_stiffness", b"1e-07")
        # (the linear pass takes it: the next refusal is the missing upload's)
        refused(L.mag_run_explicit(h, C.byref(opts(kinematics=0, rayleigh_stiffness=1e-7))), MAG_ERR_STATE, b"mag_run_explicit before mag_upload")
        refused(L.mag_run_explicit(h, C.byref(opts(kinematics=1))), MAG_ERR_STATE, b"mag_run_explicit before mag_upload")
        # mag_internal_force
        assert L.mag_internal_force(None, dp(x), dp(f), dp(sc), 0) == MAG_ERR_BAD_ARGS
        refused(L.mag_internal_force(h, None, dp(f), dp(sc), 0), MAG_ERR_BAD_ARGS, b"mag_internal_force", b"null u")
        refused(L.mag_internal_force(h, dp(x), None, dp(sc), 0), MAG_ERR_BAD_ARGS, b"mag_internal_force", b"null f_out")
        refused(L.mag_internal_force(h, dp(x), dp(f), None, 0), MAG_ERR_BAD_ARGS, b"mag_internal_force", b"null scalars_out")
        for memory in (-1, 2, 7):
            refused(L.mag_internal_force(h, dp(x), dp(f), dp(sc), memory), MAG_ERR_BAD_ARGS, b"mag_internal_force", b"mag_memory",
                    str(memory).encode())
        for memory in (_lib.MAG_MEM_HOST, _lib.MAG_MEM_DEVICE):
            refused(L.mag_internal_force(h, dp(x), dp(f), dp(sc), memory), MAG_ERR_STATE, b"mag_internal_force before mag_upload")
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        refused(L.mag_internal_force(h, dp(x), dp(f), dp(sc), 0), MAG_ERR_BAD_ARGS, b"mag_internal_force", b"communicator")
    finally:
        L.mag_destroy(h)
    for kw, word in ((dict(assemble_csr=0), b"assemble_csr = 0"), (dict(precision=1), b"precision = 1")):
        o = _lib.Options()
        L.mag_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        h = L.mag_create(C.byref(o))
        assert h
        try:
            assert L.mag_internal_force(h, dp(x), dp(f), dp(sc), 0) == MAG_ERR_STATE
            assert b"mag_internal_force" in L.mag_last_error(h) and word in L.mag_last_error(h)
        finally:
            L.mag_destroy(h)


def test_python_mirror_refuses_an_unknown_kinematics_before_the_library(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context(device=0) as c:
        c.N = 4
        for call in (lambda: c.run_explicit(4, density=RHO, kinematics="nonlinear"), lambda: c.explicit(steps=4, density=RHO, kinematics="TL"),
                     lambda: c.run_explicit(4, kinematics=1)):
            with pytest.raises(ValueError, match="kinematics"):
                call()
        with pytest.raises(MagnetiteError, match="5 entries where 8"):
            c.internal_force(np.zeros(5))
