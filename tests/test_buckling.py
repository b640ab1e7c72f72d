"""No GPU: the ABI of the buckling analysis (struct sizes, symbols, errors before any HIP call, the Python wrappers' own argument
checks) and the reference module tests/buckling_ref.py against closed forms: Euler's column, the symmetry and the kernel of K_G, its
linearity in the prestress, and the numpy subspace iteration against the dense factors on every part of the GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import buckling_ref as ref
import modal_ref
from magnetite_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
SYMBOLS = ("mag_run_buckling", "mag_download_buckling", "mag_get_buckling_info", "mag_get_buckling_stats", "mag_apply_geometric",
           "mag_assemble_geometric")


def test_abi_structs_and_symbols(built):
    assert C.sizeof(_lib.BucklingOptions) == 40 and C.sizeof(_lib.BucklingResult) == 32
    offsets = {name: getattr(_lib.BucklingOptions, name).offset for name, _ in _lib.BucklingOptions._fields_}
    assert offsets == dict(modes=0, subspace=4, max_outer=8, set=12, member=16, reserved=20, tol=24, cg_tol=32)
    offsets = {name: getattr(_lib.BucklingResult, name).offset for name, _ in _lib.BucklingResult._fields_}
    assert offsets == dict(load_factor_out=0, residual_out=8, shapes_out=16, memory=24, reserved=28)
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert "} mag_buckling_options;" in header and "} mag_buckling_result;" in header
    from magnetite_amd import Context
    for method in ("run_buckling", "download_buckling", "buckling_info", "buckling_stats", "apply_geometric", "assemble_geometric", "buckling"):
        assert callable(getattr(Context, method)), method
    assert Context.BUCKLING_INFO == ("modes", "subspace", "outer", "converged", "vectors_per_launch", "launches", "redone", "positive")


def test_struct_layouts_match_the_header(built, tmp_path):
    import subprocess
    structs = {"mag_buckling_options": _lib.BucklingOptions, "mag_buckling_result": _lib.BucklingResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "magnetite_hip.h"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        def opts(**kw):
            return _lib.BucklingOptions(**{**dict(modes=4), **kw})

        def run(o):
            return L.mag_run_buckling(h, C.byref(o) if o is not None else None)

        out, st, info, x = _lib.BucklingResult(), _lib.Stats(), (C.c_int32 * 8)(), (C.c_double * 4)()
        assert L.mag_run_buckling(None, C.byref(opts())) == MAG_ERR_BAD_ARGS
        assert L.mag_download_buckling(None, C.byref(out)) == MAG_ERR_BAD_ARGS
        assert L.mag_get_buckling_info(None, info) == MAG_ERR_BAD_ARGS
        assert L.mag_get_buckling_stats(None, 0, C.byref(st)) == MAG_ERR_BAD_ARGS
        assert L.mag_apply_geometric(None, 0, 0, x, x, 0) == MAG_ERR_BAD_ARGS
        assert L.mag_assemble_geometric(None, 0, 0, x, 0) == MAG_ERR_BAD_ARGS
        assert run(None) == MAG_ERR_BAD_ARGS and b"null options" in L.mag_last_error(h)
        for modes in (0, -3):
            assert run(opts(modes=modes)) == MAG_ERR_BAD_ARGS and b"mag_run_buckling: modes = " in L.mag_last_error(h)
        for kw in (dict(subspace=3), dict(subspace=33), dict(subspace=-1), dict(modes=30), dict(modes=33, subspace=33)):
            assert run(opts(**kw)) == MAG_ERR_BAD_ARGS, kw
            assert b"subspace = " in L.mag_last_error(h)
        assert run(opts(max_outer=-1)) == MAG_ERR_BAD_ARGS and b"max_outer" in L.mag_last_error(h)
        for key in ("tol", "cg_tol"):
            for v in (-1e-9, float("nan"), float("inf")):
                assert run(opts(**{key: v})) == MAG_ERR_BAD_ARGS, (key, v)
                assert b"cg_tol" in L.mag_last_error(h)
        for bad_set in (-1, 2, 3):  # (2: variants are no prestress)
            assert run(opts(set=bad_set)) == MAG_ERR_BAD_ARGS and b"set " in L.mag_last_error(h), bad_set
            assert L.mag_apply_geometric(h, bad_set, 0, x, x, 0) == MAG_ERR_BAD_ARGS and b"set " in L.mag_last_error(h)
            assert L.mag_assemble_geometric(h, bad_set, 0, x, 0) == MAG_ERR_BAD_ARGS and b"set " in L.mag_last_error(h)
        assert L.mag_apply_geometric(h, 0, 0, None, x, 0) == MAG_ERR_BAD_ARGS and b"null vector" in L.mag_last_error(h)
        assert L.mag_apply_geometric(h, 0, 0, x, None, 0) == MAG_ERR_BAD_ARGS
        assert L.mag_assemble_geometric(h, 0, 0, None, 0) == MAG_ERR_BAD_ARGS and b"null values_out" in L.mag_last_error(h)
        assert L.mag_assemble_geometric(h, 0, 0, x, 7) == MAG_ERR_BAD_ARGS and b"memory = 7" in L.mag_last_error(h)
        # no upload
        for o in (opts(), opts(modes=1), opts(subspace=32), opts(modes=24), opts(set=1, member=3)):
            assert run(o) == MAG_ERR_STATE and b"mag_run_buckling before mag_upload" in L.mag_last_error(h)
        assert L.mag_apply_geometric(h, 0, 0, x, x, 1) == MAG_ERR_STATE and b"before mag_upload" in L.mag_last_error(h)
        assert L.mag_assemble_geometric(h, 1, 0, x, 0) == MAG_ERR_STATE and b"before mag_upload" in L.mag_last_error(h)
        assert L.mag_download_buckling(h, None) == MAG_ERR_BAD_ARGS and b"null buckling result" in L.mag_last_error(h)
        assert L.mag_download_buckling(h, C.byref(out)) == MAG_ERR_STATE and b"before a completed mag_run_buckling" in L.mag_last_error(h)
        assert L.mag_get_buckling_info(h, None) == MAG_ERR_BAD_ARGS and L.mag_get_buckling_info(h, info) == MAG_ERR_STATE
        assert L.mag_get_buckling_stats(h, 0, None) == MAG_ERR_BAD_ARGS and L.mag_get_buckling_stats(h, -1, C.byref(st)) == MAG_ERR_BAD_ARGS
        assert L.mag_get_buckling_stats(h, 0, C.byref(st)) == MAG_ERR_STATE
        # a communicator of more than one rank
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        assert run(opts()) == MAG_ERR_BAD_ARGS and b"communicator" in L.mag_last_error(h)
        assert L.mag_apply_geometric(h, 0, 0, x, x, 0) == MAG_ERR_BAD_ARGS and b"communicator" in L.mag_last_error(h)
        assert L.mag_assemble_geometric(h, 0, 0, x, 0) == MAG_ERR_BAD_ARGS and b"communicator" in L.mag_last_error(h)
        assert L.mag_download_buckling(h, C.byref(out)) == MAG_ERR_BAD_ARGS and b"communicator" in L.mag_last_error(h)
        assert L.mag_get_buckling_info(h, info) == MAG_ERR_BAD_ARGS and L.mag_get_buckling_stats(h, 0, C.byref(st)) == MAG_ERR_BAD_ARGS
    finally:
        L.mag_destroy(h)


def test_the_python_wrappers_check_their_arguments(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        for call in (lambda: c.buckling(set="variants"), lambda: c.run_buckling(set="modal"), lambda: c.apply_geometric(np.zeros(4), set="variants"),
                     lambda: c.assemble_geometric(set=1), lambda: c.buckling(member=-1), lambda: c.buckling(member=0.5),
                     lambda: c.apply_geometric(np.zeros(4), member=-2)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.kind == "Solver" and e.value.code is None  # (the wrapper's own refusal: the library was not asked)
        with pytest.raises(MagnetiteError) as e:
            c.buckling(modes=2)
        assert e.value.code == MAG_ERR_STATE
        with pytest.raises(MagnetiteError) as e:
            c.buckling(modes=0)
        assert e.value.code == MAG_ERR_BAD_ARGS
        for call in (c.download_buckling, c.buckling_info, lambda: c.buckling_stats(0)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE


# ---- the reference module against closed forms

def test_the_twin_against_eulers_column():
    """lambda_1 P against pi^2 E I / (4 L^2) for the 16:1 cantilever column under edge compression: linear triangles lock in
    bending, so the ratio comes down from above, by a factor of about 4 in its excess per halving (1.867, 1.216, 1.052)."""
    ratios = []
    for nx, ny in ((32, 2), (64, 4), (128, 8)):
        prob = ref.column(nx, ny, 16.0, 1.0, 1.0)
        K, free, u0 = ref.linear(prob)
        lam, _ = ref.factors(K, ref.geometric_of(prob, u0), free, 1)
        ratios.append(float(lam[0] / ref.euler_load(prob, 16.0, 1.0)))
    print("lambda_1 / Euler:", ratios)
    assert ratios[0] > ratios[1] > ratios[2]
    assert 1.0 < ratios[2] <= 1.06
    assert np.allclose(ratios, [1.867, 1.216, 1.052], atol=1e-3)


@pytest.mark.parametrize("name", list(ref.TABLE))
def test_the_geometric_stiffness_is_symmetric_linear_and_blind_to_translations(name):
    prob, K, KG, free, u0, lam, _ = ref.cached(name)
    scale = abs(KG).max()
    assert abs(KG - KG.T).max() <= 1e-13 * scale
    n = KG.shape[0]
    for d in (0, 1):  # a rigid translation
        r = np.zeros(n)
        r[d::2] = 1.0
        assert np.max(np.abs(KG @ r)) <= 1e-12 * scale
    assert abs(KG[0::2][:, 1::2]).max() == 0.0  # (h_kl I_2: the directions do not couple)
    alpha = -2.5
    assert abs(ref.geometric_of(prob, alpha * u0) - alpha * KG).max() <= 1e-13 * abs(alpha) * scale


def test_doubling_the_loads_halves_the_factors():
    prob, K, KG, free, u0, lam, _ = ref.cached("frontal_mix")
    K2, free2, u2 = ref.linear(prob, 2.0 * prob.u_in, 2.0 * prob.f_in)
    lam2, _ = ref.factors(K2, ref.geometric_of(prob, u2), free2, 6)
    assert np.max(np.abs(2.0 * lam2 / lam[:6] - 1.0)) <= 1e-9


def test_the_recorded_factors_of_frontal_mix():
    lam = ref.cached("frontal_mix")[5]
    assert np.allclose(lam[:5], ref.FRONTAL_MIX, rtol=0, atol=5e-3)
    assert (np.sign(lam[:6]) == [1, 1, 1, -1, 1, 1]).all()
    assert np.all(ref.cached("holes_pull")[5] < 0) and np.all(ref.cached("column16")[5] > 0)


@pytest.mark.parametrize("name,p,q", ref.CASES)
def test_the_numpy_iteration_reaches_the_dense_factors(name, p, q):
    prob, K, KG, free, u0, lam, Phi = ref.cached(name)
    X0 = modal_ref.start_vectors(prob.mesh.xy, prob.u_known, q)
    out = ref.subspace_iteration(K, KG, free, X0, p, tol=1e-10, max_outer=ref.MAX_OUTER)
    err = float(np.max(np.abs(out["lam"] - lam[:p]) / np.abs(lam[:p])))
    ortho = ref.k_orthonormality(K, out["shapes"])
    mac = [1.0 - abs(float(Phi[k] @ (K @ out["shapes"][k]))) for k in range(p)]
    print(name, p, q, "outer", out["outer"], "err", err, "ortho", ortho, "1-MAC", max(mac))
    assert out["converged"] == 1 and out["outer"] == ref.TABLE[name][(p, q)] <= ref.MAX_OUTER
    assert err <= 1e-9
    assert ortho <= 1e-10  # (the bar of the device's shapes, here against the K the twin normalises by)
    assert max(mac) <= 1e-8
    assert np.all(np.diff(np.abs(out["lam"])) >= 0) and (np.sign(out["lam"]) == np.sign(lam[:p])).all()
