"""No GPU: the ABI of the modal analysis (struct sizes, symbols, errors before any HIP call), the host-only Rayleigh-Ritz step of
csrc/modal_host.h through a stand-alone program, and the reference module against closed forms."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import modal_ref as ref
from magnetite_amd import _lib, meshgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
SYMBOLS = ("mag_run_modal", "mag_download_modal", "mag_get_modal_info", "mag_get_modal_stats", "mag_apply_mass")


def test_abi_structs_and_symbols(built):
    assert C.sizeof(_lib.ModalOptions) == 40 and C.sizeof(_lib.ModalResult) == 40
    offsets = {name: getattr(_lib.ModalOptions, name).offset for name, _ in _lib.ModalOptions._fields_}
    assert offsets == dict(modes=0, subspace=4, max_outer=8, lumped=12, density=16, tol=24, cg_tol=32)
    offsets = {name: getattr(_lib.ModalResult, name).offset for name, _ in _lib.ModalResult._fields_}
    assert offsets == dict(lambda_out=0, frequency_out=8, residual_out=16, shapes_out=24, memory=32, reserved=36)
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4 and "MAG_ABI_VERSION 4" in header
    assert "} mag_modal_options;" in header and "} mag_modal_result;" in header
    from magnetite_amd import Context
    for method in ("run_modal", "download_modal", "modal_info", "modal_stats", "apply_mass", "modal"):
        assert callable(getattr(Context, method)), method


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        def opts(**kw):
            return _lib.ModalOptions(**{**dict(modes=4, density=2700.0), **kw})

        def run(o):
            return L.mag_run_modal(h, C.byref(o) if o is not None else None)

        out, st, info, x = _lib.ModalResult(), _lib.Stats(), (C.c_int32 * 8)(), (C.c_double * 4)()
        assert L.mag_run_modal(None, C.byref(opts())) == MAG_ERR_BAD_ARGS
        assert L.mag_download_modal(None, C.byref(out)) == MAG_ERR_BAD_ARGS
        assert L.mag_get_modal_info(None, info) == MAG_ERR_BAD_ARGS
        assert L.mag_get_modal_stats(None, 0, C.byref(st)) == MAG_ERR_BAD_ARGS
        assert L.mag_apply_mass(None, 2700.0, 0, x, x, 0) == MAG_ERR_BAD_ARGS
        assert run(None) == MAG_ERR_BAD_ARGS and b"null options" in L.mag_last_error(h)
        for modes in (0, -3):
            assert run(opts(modes=modes)) == MAG_ERR_BAD_ARGS and b"modes = " in L.mag_last_error(h)
        for kw in (dict(subspace=3), dict(subspace=33), dict(subspace=-1), dict(modes=30), dict(modes=33, subspace=33)):
            assert run(opts(**kw)) == MAG_ERR_BAD_ARGS, kw
            assert b"subspace = " in L.mag_last_error(h)
        assert run(opts(max_outer=-1)) == MAG_ERR_BAD_ARGS and b"max_outer" in L.mag_last_error(h)
        for density in (0.0, -1.0, float("nan"), float("inf")):
            assert run(opts(density=density)) == MAG_ERR_BAD_ARGS, density
            assert b"density" in L.mag_last_error(h)
            assert L.mag_apply_mass(h, density, 0, x, x, 0) == MAG_ERR_BAD_ARGS and b"density" in L.mag_last_error(h)
        for key in ("tol", "cg_tol"):
            for v in (-1e-9, float("nan"), float("inf")):
                assert run(opts(**{key: v})) == MAG_ERR_BAD_ARGS, (key, v)
                assert b"cg_tol" in L.mag_last_error(h)
        assert L.mag_apply_mass(h, 2700.0, 0, None, x, 0) == MAG_ERR_BAD_ARGS and b"null vector" in L.mag_last_error(h)
        assert L.mag_apply_mass(h, 2700.0, 0, x, None, 0) == MAG_ERR_BAD_ARGS
        # no upload
        for o in (opts(), opts(modes=1), opts(subspace=32), opts(modes=24)):
            assert run(o) == MAG_ERR_STATE and b"mag_run_modal before mag_upload" in L.mag_last_error(h)
        assert L.mag_apply_mass(h, 2700.0, 1, x, x, 1) == MAG_ERR_STATE and b"before mag_upload" in L.mag_last_error(h)
        assert L.mag_download_modal(h, None) == MAG_ERR_BAD_ARGS and b"null modal result" in L.mag_last_error(h)
        assert L.mag_download_modal(h, C.byref(out)) == MAG_ERR_STATE and b"before a completed mag_run_modal" in L.mag_last_error(h)
        assert L.mag_get_modal_info(h, None) == MAG_ERR_BAD_ARGS and L.mag_get_modal_info(h, info) == MAG_ERR_STATE
        assert L.mag_get_modal_stats(h, 0, None) == MAG_ERR_BAD_ARGS and L.mag_get_modal_stats(h, -1, C.byref(st)) == MAG_ERR_BAD_ARGS
        assert L.mag_get_modal_stats(h, 0, C.byref(st)) == MAG_ERR_STATE
        # a communicator of more than one rank
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        assert run(opts()) == MAG_ERR_BAD_ARGS and b"communicator" in L.mag_last_error(h)
        assert L.mag_apply_mass(h, 2700.0, 0, x, x, 0) == MAG_ERR_BAD_ARGS and b"communicator" in L.mag_last_error(h)
        assert L.mag_download_modal(h, C.byref(out)) == MAG_ERR_BAD_ARGS and b"communicator" in L.mag_last_error(h)
        assert L.mag_get_modal_info(h, info) == MAG_ERR_BAD_ARGS and L.mag_get_modal_stats(h, 0, C.byref(st)) == MAG_ERR_BAD_ARGS
    finally:
        L.mag_destroy(h)


def test_python_mirror_asks_for_a_density(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        with pytest.raises(MagnetiteError):
            c.modal(modes=2)
        with pytest.raises(MagnetiteError) as e:
            c.modal(modes=2, density=2700.0)
        assert e.value.code == MAG_ERR_STATE
        for call in (c.download_modal, c.modal_info, lambda: c.modal_stats(0)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE


# ---- csrc/modal_host.h through tests/cpp/modal_eig.cpp

def _sanitizer_flags(tmp_path):
    """-fsanitize=address,undefined where a trial link of an empty program with it works, else nothing (said in the output)."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    trial = subprocess.run(["g++", *flags, str(empty), "-o", str(tmp_path / "empty")], capture_output=True, text=True)
    if trial.returncode == 0 and subprocess.run([str(tmp_path / "empty")], capture_output=True).returncode == 0:
        return flags
    print("modal_eig: the sanitizers do not link here; built without them:", trial.stderr[-300:])
    return []


def _parse(text):
    """[(n, status, pivot, dict(A, B, lambda, Q))] of the program's output"""
    pairs = []
    for line in text.splitlines():
        word, *rest = line.split()
        if word == "pair":
            pairs.append((int(rest[0]), int(rest[2]), int(rest[4]), {}))
        else:
            pairs[-1][3][word] = np.array([float.fromhex(t) for t in rest])
    return pairs


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_rayleigh_ritz_step_on_the_host(tmp_path):
    exe = tmp_path / "modal_eig"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *_sanitizer_flags(tmp_path), "-I", os.path.join(ROOT, "magnetite_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "modal_eig.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    first = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert first.returncode == 0, (first.stdout[-500:], first.stderr[-3000:])
    again = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert again.stdout == first.stdout  # a repeat: the same bits
    pairs = _parse(first.stdout)
    assert [p[0] for p in pairs] == [1, 2, 7, 12, 32, 4, 3]
    for n, status, pivot, m in pairs[:-1]:
        assert status == 0
        A, B, lam, Q = m["A"].reshape(n, n), m["B"].reshape(n, n), m["lambda"], m["Q"].reshape(n, n)
        resid = np.max(np.abs(A @ Q - B @ Q @ np.diag(lam)))
        ortho = np.max(np.abs(Q.T @ B @ Q - np.eye(n)))
        print("n", n, "|A Q - B Q L|", resid, "|A|", np.max(np.abs(A)), "|Q^T B Q - I|", ortho)
        assert resid <= 1e-12 * np.max(np.abs(A))
        assert ortho <= 1e-12
        assert np.all(np.diff(lam) >= 0)
        for k in range(n):  # the sign convention
            assert Q[int(np.argmax(np.abs(Q[:, k]))), k] > 0
        want = np.sort(np.linalg.eigvals(np.linalg.solve(B, A)).real)
        assert np.max(np.abs(lam - want) / want) <= 1e-10
    n, status, pivot, m = pairs[5]
    assert np.allclose(m["lambda"], [3.0, 3.0, 5.0, 7.0], rtol=1e-14) and abs(m["lambda"][0] - m["lambda"][1]) <= 1e-14  # two equal eigenvalues
    n, status, pivot, m = pairs[-1]
    assert status == 2 and pivot == 2 and "lambda" not in m  # the rank-deficient B: reported, not factored


# ---- the reference module against closed forms

@pytest.mark.parametrize("lumped", [False, True])
def test_reference_mass_sums_to_the_parts_mass(lumped):
    mesh = meshgen.plate_with_holes(12)
    rho, t = 2700.0, 0.37
    M = ref.mass(mesh.xy, mesh.conn, rho, t, lumped)
    area = np.abs(ref.signed_areas(mesh.xy, mesh.conn)).sum()
    ones = np.ones(2 * mesh.num_nodes)
    assert abs(ones @ (M @ ones) - 2 * rho * t * area) <= 1e-12 * rho * t * area
    x_only = np.zeros(2 * mesh.num_nodes)
    x_only[0::2] = 1.0
    assert abs(x_only @ (M @ x_only) - rho * t * area) <= 1e-12 * rho * t * area
    assert abs(M - M.T).max() == 0.0
    flipped = ref.mass(mesh.xy, meshgen.clockwise(mesh).conn, rho, t, lumped)  # |A|: the orientation does not matter
    assert abs(flipped - M).max() <= 1e-12 * abs(M).max()


def test_reference_stiffness_has_the_rigid_body_modes_and_the_prototype_converges():
    prob = meshgen.config_fixed_left_pull_right(meshgen.plate(8))
    K, M, free = ref.matrices(prob, 2700.0)
    xy = prob.mesh.xy
    n = 2 * prob.mesh.num_nodes
    tx, ty, rot = np.zeros(n), np.zeros(n), np.zeros(n)
    tx[0::2], ty[1::2] = 1.0, 1.0
    rot[0::2], rot[1::2] = -xy[:, 1], xy[:, 0]
    scale = abs(K).max()
    for v in (tx, ty, rot):
        assert np.max(np.abs(K @ v)) <= 1e-12 * scale
    assert abs(K - K.T).max() <= 1e-12 * scale
    lam, Phi = ref.eigenpairs(K, M, free, k=6)
    out = ref.subspace_iteration(K, M, free, ref.start_vectors(xy, prob.u_known, 12), 6)
    assert out["converged"] == 1 and out["outer"] <= 40
    assert np.max(np.abs(out["lam"] - lam) / lam) <= 1e-8
    assert max(ref.true_residual(K, M, free, out["lam"][k], out["shapes"][k]) for k in range(6)) <= 1e-4
    assert max(ref.true_residual(K, M, free, lam[k], Phi[k]) for k in range(6)) <= 1e-9
