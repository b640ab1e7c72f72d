"""CPU: the element stiffness field and the density design update -- the ABI of the new entry points, their argument and
call-order errors (all before any HIP call), and the numpy twin against itself: its gradients against central differences of
re-solved problems, the filter's identities, and the twenty-iteration runs whose trajectory the GPU test compares with.

(The refusals WHILE A FIELD IS SET cannot be reached here: setting a field needs an upload, which needs a device.  They are in
tests/test_design_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adjoint_ref as aref
import design_ref as dref
from magnetite_amd import _lib, meshgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
SYMBOLS = ("mag_set_element_scale", "mag_design_init", "mag_design_step", "mag_get_design_info", "mag_download_design")


def test_struct_sizes_symbols_and_header(built, tmp_path):
    assert C.sizeof(_lib.DesignOptions) == 48 and C.sizeof(_lib.Design) == 40
    offsets = {name: getattr(_lib.DesignOptions, name).offset for name, _ in _lib.DesignOptions._fields_}
    assert offsets == dict(volume_fraction=0, scale_min=8, rho_min=16, move=24, penal=32, filter_passes=36, reserved=40)
    offsets = {name: getattr(_lib.Design, name).offset for name, _ in _lib.Design._fields_}
    assert offsets == dict(rho_out=0, rho_filtered_out=8, scale_out=16, dJ_drho_out=24, memory=32, reserved=36)
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "magnetite_hip.h"\n'
                   'int main(void){printf("%zu %zu\\n", sizeof(mag_design_options), sizeof(mag_design));return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["48", "40"]
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    exported = set(re.findall(r" T (mag_[a-z_0-9]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH], text=True)))
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS and name in exported
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4 and "MAG_ABI_VERSION 4" in header
    assert "} mag_design_options;" in header and "} mag_design;" in header


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        good = lambda **kw: _lib.DesignOptions(**{**dict(volume_fraction=0.5, scale_min=1e-3, rho_min=1e-3, move=0.2, penal=3, filter_passes=1), **kw})
        info, out, s = (C.c_double * 8)(), _lib.Design(), (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
        assert L.mag_set_element_scale(None, s, 0) == MAG_ERR_BAD_ARGS
        assert L.mag_design_init(None, C.byref(good()), None, 0) == MAG_ERR_BAD_ARGS
        assert L.mag_design_step(None, None, 0) == MAG_ERR_BAD_ARGS
        assert L.mag_get_design_info(None, info) == MAG_ERR_BAD_ARGS
        assert L.mag_download_design(None, C.byref(out)) == MAG_ERR_BAD_ARGS
        assert L.mag_design_init(h, None, None, 0) == MAG_ERR_BAD_ARGS and b"null options" in L.mag_last_error(h)
        nan, inf = float("nan"), float("inf")
        bad = dict(volume_fraction=(0.0, -0.1, 1.0000001, nan, inf), scale_min=(0.0, 1.0, -1e-3, nan), rho_min=(0.0, 1.0, 2.0, nan),
                   move=(0.0, -0.2, 1.5, nan, inf), penal=(0, 9, -1), filter_passes=(-1, 9))
        for field, values in bad.items():
            for v in values:
                assert L.mag_design_init(h, C.byref(good(**{field: v})), None, 0) == MAG_ERR_BAD_ARGS, (field, v)
                assert field.encode() in L.mag_last_error(h), (field, v)
        for ok in (dict(volume_fraction=1.0), dict(move=1.0), dict(penal=1), dict(penal=8), dict(filter_passes=0), dict(filter_passes=8)):
            assert L.mag_design_init(h, C.byref(good(**ok)), None, 0) == MAG_ERR_STATE, ok  # in range: the upload is missed
            assert b"mag_design_init before mag_upload" in L.mag_last_error(h)
        for scale in (s, None):
            assert L.mag_set_element_scale(h, scale, 0) == MAG_ERR_STATE
            assert b"mag_set_element_scale before mag_upload" in L.mag_last_error(h)
        for memory in (-1, 2, 7):  # none of enum mag_memory: refused where the pointer would be read
            assert L.mag_set_element_scale(h, s, memory) == MAG_ERR_BAD_ARGS and b"mag_memory" in L.mag_last_error(h)
            assert L.mag_design_init(h, C.byref(good()), s, memory) == MAG_ERR_BAD_ARGS and b"mag_memory" in L.mag_last_error(h)
            assert L.mag_design_step(h, s, memory) == MAG_ERR_BAD_ARGS and b"mag_memory" in L.mag_last_error(h)
            assert L.mag_download_design(h, C.byref(_lib.Design(memory=memory))) == MAG_ERR_BAD_ARGS and b"mag_memory" in L.mag_last_error(h)
            assert L.mag_set_element_scale(h, None, memory) == MAG_ERR_STATE  # (nothing to read: the upload is missed)
        assert L.mag_design_step(h, None, 0) == MAG_ERR_STATE and b"before mag_design_init" in L.mag_last_error(h)
        assert L.mag_design_step(h, s, 0) == MAG_ERR_STATE
        assert L.mag_get_design_info(h, None) == MAG_ERR_BAD_ARGS
        assert L.mag_get_design_info(h, info) == MAG_ERR_STATE
        assert L.mag_download_design(h, None) == MAG_ERR_BAD_ARGS and b"null design" in L.mag_last_error(h)
        assert L.mag_download_design(h, C.byref(out)) == MAG_ERR_STATE and b"before mag_design_init" in L.mag_last_error(h)
    finally:
        L.mag_destroy(h)


def test_python_mirror_and_call_order(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        for call in (lambda: c.set_element_scale(np.ones(4)), lambda: c.set_element_scale(None), c.design_init, c.design_step, c.design_info,
                     c.download_design, lambda: c.design_step(np.ones(4))):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE
        with pytest.raises(MagnetiteError) as e:
            c.design_init(penal=0)
        assert e.value.code == MAG_ERR_BAD_ARGS
        assert callable(c.topopt)


# ---- the twin against itself
def fd_problem():
    """plate(6, 5): left edge fixed, right edge pulled by a nonzero prescribed displacement, seeded forces on the free DOFs"""
    import dataclasses
    prob = meshgen.config_fixed_left_pull_right(meshgen.plate(6, 5))
    free = prob.u_known == 0
    k_scale = prob.youngs_modulus * prob.part_thickness * prob.meta["delta"]
    return dataclasses.replace(prob, f_in=np.where(free, 0.05 * k_scale * np.random.default_rng(5).standard_normal(free.size), 0.0))


def check(what, got, fd_h, fd_h2, gmax):
    """tests/test_adjoint.py's bar on its finite-difference checks"""
    err, rich = abs(got - fd_h2), abs(fd_h - fd_h2)
    print(what, "got", got, "fd", fd_h2, "err/max|g|", err / gmax, "richardson/max|g|", rich / gmax)
    assert err <= 4 * rich + 2e-7 * gmax, what


def central(fn, scale, e, h):
    out = []
    for s in (h, h / 2):
        up, down = scale.copy(), scale.copy()
        up[e] += s
        down[e] -= s
        out.append((fn(up) - fn(down)) / (2 * s))
    return out


def test_the_gradients_with_respect_to_the_scale_are_those_of_central_differences():
    """dJ/ds_e = -2 energy[e] / s_e for J = -2 Pi, and delem[e] / s_e for a disp_lsq objective through the adjoint, on a dense
    solve of plate(6, 5) under s = 10^U(-2, 0)"""
    prob = fd_problem()
    E = len(prob.mesh.conn)
    assert (len(prob.mesh.xy), E) == (42, 60)
    scale = dref.random_scale(E)
    sol = dref.solve(prob, scale)
    sens = dref.sensitivities(prob, sol, scale)
    g_stiff = -2.0 * sens["energy"] / scale
    w = aref.patch_weights(prob)
    target = 0.5 * sol["u"] * np.random.default_rng(4).uniform(0.5, 1.5, sol["u"].size)
    J = lambda s: float(np.sum(w * (dref.solve(prob, s)["u"] - target) ** 2))
    adj = dref.adjoint(prob, sol["u"], 2.0 * w * (sol["u"] - target), scale)
    g_lsq = adj["delem"] / scale
    rng = np.random.default_rng(1)
    for e in rng.choice(E, 12, replace=False):
        check(("J = -2 Pi", e), g_stiff[e], *central(lambda s: -2.0 * dref.potential(prob, s), scale, e, 1e-3 * scale[e]), np.abs(g_stiff).max())
        check(("disp_lsq", e), g_lsq[e], *central(J, scale, e, 1e-3 * scale[e]), np.abs(g_lsq).max())


@pytest.mark.parametrize("name", ["plate_32x16", "frontal16", "plate_6x5"])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_the_filter_identities(name, P):
    """y . (F x) == (F^T y) . x and sum_e w_e rho_e == sum_e a_e (F^P rho)_e for positive random vectors, relative 1e-11: the sums
    have E <= 2000 positive terms, so the bound sits two orders above E 2^-53"""
    mesh = meshgen.plate(6, 5) if name == "plate_6x5" else dref.TOPOPT_MESHES[name]()
    f = dref.Filter(mesh.xy, mesh.conn)
    E = len(mesh.conn)
    assert E <= 2000 and (f.area > 0).all()
    rng = np.random.default_rng(8)
    x, y, rho = rng.uniform(0.1, 1.0, E), rng.uniform(0.1, 1.0, E), rng.uniform(1e-3, 1.0, E)
    a, b = float(y @ f.forward(x)), float(f.transpose(y) @ x)
    assert abs(a - b) <= 1e-11 * abs(a)
    w = f.passes(f.area, P, transpose=True)
    a, b = float(w @ rho), float(f.area @ f.passes(rho, P))
    print(name, P, a, b, abs(a - b) / a)
    assert abs(a - b) <= 1e-11 * abs(a)
    assert abs(float(np.sum(f.forward(np.ones(E)))) - E) <= 1e-11 * E  # F keeps a constant


# the twin's twenty iterations with direct solves: J_19 / J_0 and the largest J_{k+1} / J_k, to the four digits they are stated with
TRAJECTORY = {"plate_32x16": (1024, 561, 0.2612, 0.9944), "frontal16": (594, 332, 0.2507, 0.9989)}


@pytest.mark.parametrize("name", list(TRAJECTORY))
def test_twenty_iterations_of_the_twin(name):
    E, N, last, largest = TRAJECTORY[name]
    prob = dref.cantilever(dref.TOPOPT_MESHES[name]())
    assert (len(prob.mesh.conn), len(prob.mesh.xy)) == (E, N)
    ref = dref.reference_trajectory(name)
    J = np.array([h["J"] for h in ref["history"]])
    ratios = J[1:] / J[:-1]
    print(name, "J19/J0", J[-1] / J[0], "largest ratio", ratios.max(), "volume errors", max(abs(h["volume_fraction"] - 0.5) for h in ref["history"]))
    assert len(J) == 20 and (J > 0).all()
    assert abs(J[-1] / J[0] - last) <= 5e-5 and abs(ratios.max() - largest) <= 5e-5
    assert (ratios < 1.0).all()
    for h in ref["history"]:
        assert abs(h["volume_fraction"] - 0.5) <= 1.2e-16 and h["reachable"] == 1 and 0 < h["change"] <= 0.2 * (1 + 2.0 ** -50)
    assert (ref["rho"] >= 1e-3).all() and (ref["rho"] <= 1.0).all()
    two = dref.topopt(prob, 20, filter_passes=2)["history"]
    print(name, "two filter passes", two[-1]["J"] / two[0]["J"])
    assert abs(two[-1]["J"] / two[0]["J"] - {"plate_32x16": 0.2982, "frontal16": 0.2733}[name]) <= 5e-5
