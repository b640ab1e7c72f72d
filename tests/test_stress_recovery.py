"""CPU: the reference of the stress recovery tests passes the patch test (a constant stress is recovered at every node, the
error estimate vanishes, on clockwise elements too); its ZZ estimate tracks the true error of an interpolated quadratic field
(effectivity near 1, first order in h); U^2 is twice the strain energy of the sensitivities and sqrt(sum vm^2) the p = 2
aggregate of the objective; the entry points exist in header, binding and library, the struct has the header's size, and every
argument and call-order error comes back before any HIP call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import objective_ref as oref
import sensitivities_ref as sref
import stress_recovery_ref as ref
from magnetite_amd import _lib, meshgen
from magnetite_amd.meshgen import ALU
from test_sensitivities import base_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
SYMBOLS = ("mag_run_stress", "mag_download_stress")
YOUNGS, NU, THICK = ALU["youngs_modulus"], ALU["poisson_ratio"], ALU["part_thickness"]

PATCH_MESHES = {
    "plate8": lambda: meshgen.plate(8),
    "holes10_shuffled": lambda: meshgen.shuffle(meshgen.plate_with_holes(10), 3),
    "frontal12": lambda: meshgen.frontal_like(12, 0.4, 2),
    "plate6_clockwise": lambda: meshgen.clockwise(meshgen.plate(6)),
}


def recover(mesh, u):
    return ref.stress_recovery(mesh.xy, mesh.conn, u, YOUNGS, NU, THICK)


@pytest.mark.parametrize("name", list(PATCH_MESHES))
def test_patch_test_a_constant_stress_is_recovered_and_the_estimate_vanishes(name):
    mesh = PATCH_MESHES[name]()
    x, y = np.asarray(mesh.xy, dtype=np.float64).reshape(-1, 2).T
    u = np.column_stack([1e-3 * x + 2e-4 * y, -3e-4 * x + 5e-4 * y]).reshape(-1)
    ex, ey, gxy = 1e-3, 5e-4, 2e-4 - 3e-4
    c = YOUNGS / (1 - NU ** 2)
    want = np.array([c * (ex + NU * ey), c * (NU * ex + ey), c * (1 - NU) / 2 * gxy])
    got = recover(mesh, u)
    dev = np.abs(got["node"][:, :3] - want).max() / np.abs(want).max()
    print(name, "nodal deviation", dev, "eta^2 / U^2", got["eta_sq"] / got["energy_sq"], "U^2", got["energy_sq"])
    assert dev <= 1e-13
    assert got["energy_sq"] > 0  # (the clockwise mesh: |A|, not the signed area)
    assert got["eta_sq"] <= 1e-24 * got["energy_sq"]
    assert abs(got["vm_max"] - ref.von_mises(want)) <= 1e-13 * ref.von_mises(want)
    assert got["eta_rel"] <= 1e-12


def quadratic_field(xy):
    x, y = xy.T
    return 1e-3 * np.column_stack([x * x + 0.5 * x * y - 0.3 * y * y + 0.2 * x, -0.4 * x * x + 0.7 * x * y + 0.6 * y * y - 0.1 * y])


def quadratic_stress(xy):
    """(N, 3): the stress of quadratic_field, linear in x and y."""
    x, y = xy.T
    ex, ey, gxy = 1e-3 * (2 * x + 0.5 * y + 0.2), 1e-3 * (0.7 * x + 1.2 * y - 0.1), 1e-3 * ((0.5 * x - 0.6 * y) + (-0.8 * x + 0.7 * y))
    c = YOUNGS / (1 - NU ** 2)
    return np.column_stack([c * (ex + NU * ey), c * (NU * ex + ey), c * (1 - NU) / 2 * gxy])


QUALITY_MESHES = {"plate": meshgen.plate, "holes": meshgen.plate_with_holes, "frontal": lambda n: meshgen.frontal_like(n, 0.4, 2)}


@pytest.mark.parametrize("family", list(QUALITY_MESHES))
def test_the_estimate_tracks_the_true_error_of_an_interpolated_quadratic_field(family):
    eta = {}
    for n in (8, 16, 32):
        mesh = QUALITY_MESHES[family](n)
        xy = np.asarray(mesh.xy, dtype=np.float64).reshape(-1, 2)
        conn = np.asarray(mesh.conn).reshape(-1, 3)
        got = recover(mesh, quadratic_field(xy).reshape(-1))
        # the true error: the same exact triangle integral with the analytic (linear) stress at the corners
        true = np.sqrt(np.sum(ref.triangle_integral(quadratic_stress(xy)[conn], got["elem"][:, :3], ref.areas(xy, conn), NU, YOUNGS, THICK)))
        eta[n] = np.sqrt(got["eta_sq"])
        print(family, n, "eta", eta[n], "true", true, "effectivity", eta[n] / true, "eta_rel", got["eta_rel"])
        assert 0.9 <= eta[n] / true <= 1.1, (family, n)
        assert abs(np.sum(got["eta2"]) - got["eta_sq"]) <= 1e-14 * got["eta_sq"] and (got["eta2"] >= 0).all()
    for n in (8, 16):
        print(family, n, "eta(n) / eta(2n)", eta[n] / eta[2 * n])
        assert 1.9 <= eta[n] / eta[2 * n] <= 2.1, (family, n)


@pytest.mark.parametrize("config", [meshgen.config_fixed_left_pull_right, meshgen.config_fixed_left_point_load])
def test_energy_norm_is_twice_the_strain_energy_and_vm_the_objectives(config):
    prob = base_problem(config)
    sol = sref.direct_solution(prob)
    got = ref.of_problem(prob, sol["u"])
    W = sref.of_solution(prob, sol)["strain_energy"]
    print(config.__name__, "U^2", got["energy_sq"], "2W", 2 * W, "rel", abs(got["energy_sq"] - 2 * W) / (2 * W))
    assert abs(got["energy_sq"] - 2 * W) <= 1e-12 * 2 * W
    J = oref.of_problem("stress_pnorm", prob, sol["u"], p=2.0, scale=1.0)["J"]
    l2 = np.sqrt(np.sum(got["elem"][:, 3] ** 2))
    print(config.__name__, "sqrt(sum vm^2)", l2, "J(p = 2)", J, "rel", abs(l2 - J) / J)
    assert abs(l2 - J) <= 1e-13 * J
    assert got["vm_max"] == got["elem"][:, 3].max() and got["vm_node_max"] == got["node"][:, 3].max()


def test_a_node_that_no_element_touches_gets_zeros():
    xy = np.array([[0, 0], [1, 0], [0, 1], [5, 5]], dtype=np.float64)
    got = ref.stress_recovery(xy, np.array([[0, 1, 2]], dtype=np.int32), 1e-3 * np.arange(8.0), YOUNGS, NU, THICK)
    assert not got["node"][3].any() and got["node"][:3, 3].min() > 0
    assert np.abs(got["node"][:3] - got["elem"][0]).max() <= 1e-15 * np.abs(got["elem"][0]).max()
    none = ref.stress_recovery(xy, np.array([[0, 1, 2]], dtype=np.int32), np.zeros(8), YOUNGS, NU, THICK)
    assert none["eta_rel"] == 0.0 and none["eta_sq"] == 0.0 and none["energy_sq"] == 0.0


def test_struct_size_symbols_and_header(built, tmp_path):
    assert C.sizeof(_lib.StressField) == 96
    offsets = {name: getattr(_lib.StressField, name).offset for name, _ in _lib.StressField._fields_}
    assert offsets == dict(elem_out=0, node_out=8, eta2_out=16, scalars=24, memory=88, reserved=92)
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "magnetite_hip.h"\nint main(void){printf("%zu\\n", sizeof(mag_stress_field));return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)], text=True)) == 96
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    exported = set(re.findall(r" T (mag_[a-z_0-9]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH], text=True)))
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS and name in exported
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4 and "MAG_ABI_VERSION 4" in header
    assert "} mag_stress_field;" in header


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        o = _lib.StressField()
        assert L.mag_run_stress(None, 0) == MAG_ERR_BAD_ARGS
        assert L.mag_download_stress(None, 0, 0, C.byref(o)) == MAG_ERR_BAD_ARGS
        for bad in (-1, 3, 99):
            assert L.mag_run_stress(h, bad) == MAG_ERR_BAD_ARGS
            assert b"mag_set" in L.mag_last_error(h)
            assert L.mag_download_stress(h, bad, 0, C.byref(o)) == MAG_ERR_BAD_ARGS
            assert b"mag_set" in L.mag_last_error(h)
        for s, fn in ((0, b"mag_run"), (1, b"mag_run_cases"), (2, b"mag_run_variants")):
            assert L.mag_run_stress(h, s) == MAG_ERR_STATE  # no completed run of that set
            assert b"mag_run_stress before a completed " + fn in L.mag_last_error(h)
            assert L.mag_download_stress(h, s, 0, None) == MAG_ERR_BAD_ARGS
            assert b"null stress field" in L.mag_last_error(h)
            assert L.mag_download_stress(h, s, -1, C.byref(o)) == MAG_ERR_BAD_ARGS
            assert b"out of range" in L.mag_last_error(h)
            assert L.mag_download_stress(h, s, 0, C.byref(o)) == MAG_ERR_STATE
            assert fn in L.mag_last_error(h)
        # a communicator of more than one rank
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        for s in (0, 1, 2):
            assert L.mag_run_stress(h, s) == MAG_ERR_BAD_ARGS
            assert b"communicator" in L.mag_last_error(h)
            assert L.mag_download_stress(h, s, 0, C.byref(o)) == MAG_ERR_BAD_ARGS
            assert b"communicator" in L.mag_last_error(h)
    finally:
        L.mag_destroy(h)


def test_python_mirror_names_the_sets(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        with pytest.raises(MagnetiteError):
            c.stress_recovery("all")
        for s in ("run", "cases", "variants"):
            with pytest.raises(MagnetiteError) as e:
                c.stress_recovery(s)
            assert e.value.code == MAG_ERR_STATE
            with pytest.raises(MagnetiteError) as e:
                c.download_stress(s, 0)
            assert e.value.code == MAG_ERR_STATE
