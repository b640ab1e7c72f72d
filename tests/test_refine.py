"""CPU: the numpy twin of mag_run_refine (tests/refine_ref.py) keeps the invariants of a conforming longest-edge refinement over
five successive refinements of every mesh family -- no hanging node, the area, every child's orientation, the smallest angle --,
marks exactly what the header's rules say (ties, -0.0, a zero maximum); the entry points exist in header, binding and library,
the two structs have the header's sizes, and every argument and call-order error comes back before any HIP call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import refine_ref as ref
from magnetite_amd import _lib, meshgen
from magnetite_amd.meshgen import Mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
SYMBOLS = ("mag_run_refine", "mag_get_refine_info", "mag_download_refine", "mag_upload_refined")
L_SHAPE = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], dtype=np.float64)

MESHES = {
    "plate8": lambda: meshgen.plate(8),
    "holes24": lambda: meshgen.plate_with_holes(24),
    "frontal24": lambda: meshgen.frontal_like(24),
    "holes16_perturbed": lambda: meshgen.perturb(meshgen.plate_with_holes(16), 0.2),
    "frontal12_clockwise": lambda: meshgen.clockwise(meshgen.frontal_like(12)),
    "l_shape": lambda: meshgen.polygon_mesh(L_SHAPE, 0.15),
    "tie_strip16": lambda: ref.tie_strip(16),
}


def marks_of(kind, xy, conn, rng):
    if kind == "random":
        return rng.random(len(conn)) < 0.1
    c = xy[conn].mean(axis=1)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    d = np.hypot(*(c - (lo + 0.37 * (hi - lo))).T)
    return d <= np.quantile(d, 0.15)


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("kind", ["random", "near_a_point"])
@pytest.mark.parametrize("name", list(MESHES))
def test_five_successive_refinements_keep_the_invariants(name, kind, split):
    mesh = MESHES[name]()
    xy, conn = np.asarray(mesh.xy, dtype=np.float64), np.asarray(mesh.conn, dtype=np.int32)
    rng = np.random.default_rng(5)
    area0, angle0 = ref.signed_area2(xy, conn).sum(), ref.min_angle_deg(xy, conn)
    sign0 = np.sign(ref.signed_area2(xy, conn))
    assert (sign0 == sign0[0]).all()
    ref.assert_conforming(conn)
    for it in range(5):
        out = ref.free_mesh(Mesh(xy, conn), marks=marks_of(kind, xy, conn, rng), split=split)
        nxy, nconn = out["xy"], out["conn"]
        ref.assert_conforming(nconn, conn, out["node_parents"])
        a2 = ref.signed_area2(nxy, nconn)
        assert abs(a2.sum() - area0) <= 1e-12 * abs(area0)
        assert (np.sign(a2) == sign0[0]).all() and (np.sign(a2) == np.sign(ref.signed_area2(xy, conn))[out["elem_parent"]]).all()
        angle = ref.min_angle_deg(nxy, nconn)
        print(name, kind, split, "round", it, "E", len(conn), "->", len(nconn), "sweeps", out["sweeps"], "smallest angle", angle0, "->", angle)
        assert angle >= 0.5 * angle0
        assert out["nodes"] == len(nxy) == len(xy) + out["marked_edges"] and out["elements"] == len(nconn)
        assert len(nconn) == len(conn) + out["split2"] + 2 * out["split3"] + 3 * out["split4"]
        assert np.array_equal(nxy[:len(xy)], xy)
        lo, hi = out["node_parents"].T
        assert (lo < hi).all() and np.array_equal(nxy[len(xy):], 0.5 * (xy[lo] + xy[hi]))
        xy, conn = nxy, nconn


@pytest.mark.parametrize("name", list(MESHES))
def test_no_marks_change_nothing_and_all_marks_split_in_four(name):
    prob = meshgen.config_fixed_left_pull_right(MESHES[name]())
    E = prob.mesh.num_elements
    for split in (1, 3):
        same = ref.of_problem(prob, marks=np.zeros(E, dtype=np.uint8), split=split)
        assert np.array_equal(same["xy"], prob.mesh.xy) and np.array_equal(same["conn"], prob.mesh.conn)
        assert np.array_equal(same["u_known"], prob.u_known) and np.array_equal(same["u_in"], prob.u_in) and np.array_equal(same["f_in"], prob.f_in)
        assert same["sweeps"] == 1 and same["marked_edges"] == 0 and np.array_equal(same["elem_parent"], np.arange(E))
    four = ref.of_problem(prob, marks=np.ones(E, dtype=np.uint8), split=3)
    assert four["split4"] == E and four["elements"] == 4 * E and four["split2"] == four["split3"] == 0
    assert np.array_equal(four["elem_parent"], np.repeat(np.arange(E), 4))
    ref.assert_conforming(four["conn"], prob.mesh.conn, four["node_parents"])


def test_a_long_closure_on_the_tie_strip():
    """Every slanted edge of the strip has len2 = 4.25 exactly: only the tie rule (the smaller edge id) orders them, and marking
    the last element walks the closure through the whole strip -- one edge per sweep."""
    mesh = ref.tie_strip(64)
    a = mesh.xy[mesh.conn]
    slanted = np.abs(a[:, 0, 1] - a[:, 2, 1]) > 0
    assert slanted.all() and set(np.sum((a - np.roll(a, -1, axis=1)) ** 2, axis=2).reshape(-1)) == {1.0, 4.25}
    marks = np.zeros(128, dtype=np.uint8)
    marks[-1] = 1
    out = ref.free_mesh(mesh, marks=marks)
    print("tie strip 64, last element marked: sweeps", out["sweeps"], "marked edges", out["marked_edges"])
    assert out["sweeps"] == 128 and out["marked_edges"] == 128 and out["marked"] == 1
    ref.assert_conforming(out["conn"], mesh.conn, out["node_parents"])
    first = ref.free_mesh(mesh, marks=marks[::-1].copy())
    assert first["sweeps"] < 8


def test_the_marking_rules():
    ind = np.array([0.5, 2.0, -0.0, 2.0, 0.0, 1.0, 2.0, 0.25])
    # top fraction: k = ceil(theta E), ties to the lower index, -0.0 is a zero and not the largest value
    assert list(np.flatnonzero(ref.mark_elements(8, indicator=ind, rule="top_fraction", theta=0.25))) == [1, 3]
    assert list(np.flatnonzero(ref.mark_elements(8, indicator=ind, rule="top_fraction", theta=0.26))) == [1, 3, 6]
    assert list(np.flatnonzero(ref.mark_elements(8, indicator=ind, rule="top_fraction", theta=1e-9))) == [1]
    assert list(np.flatnonzero(ref.mark_elements(8, indicator=ind, rule="top_fraction", theta=0.8))) == [0, 1, 2, 3, 5, 6, 7]
    assert ref.mark_elements(8, indicator=ind, rule="top_fraction", theta=1.0).all()
    # max fraction: >= theta * max; nothing when the maximum is 0
    assert list(np.flatnonzero(ref.mark_elements(8, indicator=ind, rule="max_fraction", theta=0.5))) == [1, 3, 5, 6]
    assert not ref.mark_elements(8, indicator=np.zeros(8), rule="max_fraction", theta=0.5).any()
    assert ref.mark_elements(8, indicator=np.zeros(8), rule="top_fraction", theta=0.5).sum() == 4
    for bad in (np.nan, np.inf, -1e-300):
        worse = ind.copy()
        worse[5] = bad
        with pytest.raises(ValueError, match=r"indicator\[5\]"):
            ref.mark_elements(8, indicator=worse, rule="max_fraction", theta=0.5)


def test_boundary_data_of_new_nodes():
    """Both parents prescribed: the interpolated constraint; otherwise a free node without load: the total load is preserved."""
    for config in (meshgen.config_fixed_left_pull_right, meshgen.config_fixed_left_point_load):
        prob = config(meshgen.plate(6))
        N, E = prob.mesh.num_nodes, prob.mesh.num_elements
        out = ref.of_problem(prob, marks=np.ones(E, dtype=np.uint8), split=3)
        known, u_in, f_in = out["u_known"].reshape(-1, 2), out["u_in"].reshape(-1, 2), out["f_in"].reshape(-1, 2)
        assert np.array_equal(known[:N].reshape(-1), prob.u_known) and np.array_equal(f_in[:N].reshape(-1), prob.f_in)
        assert not f_in[N:].any() and f_in.sum() == prob.f_in.sum()
        k0, u0 = prob.u_known.reshape(-1, 2), prob.u_in.reshape(-1, 2)
        lo, hi = out["node_parents"].T
        assert np.array_equal(known[N:] != 0, (k0[lo] != 0) & (k0[hi] != 0))
        assert np.array_equal(u_in[N:], np.where(known[N:] != 0, 0.5 * (u0[lo] + u0[hi]), 0.0))
        x = out["xy"][:, 0]
        assert (known[x == 0.0] == 1).all() and known[N:].any()  # the new nodes of the fixed edge are fixed


def test_struct_sizes_symbols_and_header(built, tmp_path):
    assert C.sizeof(_lib.RefineOptions) == 40 and C.sizeof(_lib.Refined) == 64
    offsets = {name: getattr(_lib.RefineOptions, name).offset for name, _ in _lib.RefineOptions._fields_}
    assert offsets == dict(rule=0, split=4, theta=8, marks=16, indicator=24, memory=32, reserved=36)
    offsets = {name: getattr(_lib.Refined, name).offset for name, _ in _lib.Refined._fields_}
    assert offsets == dict(xy=0, conn=8, u_known=16, u_in=24, f_in=32, node_parents=40, elem_parent=48, memory=56, reserved=60)
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "magnetite_hip.h"\n'
                   'int main(void){printf("%zu %zu\\n", sizeof(mag_refine_options), sizeof(mag_refined));return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["40", "64"]
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    exported = set(re.findall(r" T (mag_[a-z_0-9]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH], text=True)))
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS and name in exported
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4 and "MAG_ABI_VERSION 4" in header
    assert "} mag_refine_options;" in header and "} mag_refined;" in header
    assert (_lib.MAG_REFINE_MARKS, _lib.MAG_REFINE_MAX_FRACTION, _lib.MAG_REFINE_TOP_FRACTION) == (0, 1, 2)
    assert "MAG_REFINE_MARKS = 0, MAG_REFINE_MAX_FRACTION = 1, MAG_REFINE_TOP_FRACTION = 2" in header


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        marks = (C.c_uint8 * 4)()
        ind = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
        good = lambda **kw: _lib.RefineOptions(**{**dict(rule=0, split=1, theta=0.2, marks=C.addressof(marks), indicator=C.addressof(ind)), **kw})
        info, out = (C.c_int64 * 8)(), _lib.Refined()
        assert L.mag_run_refine(None, C.byref(good())) == MAG_ERR_BAD_ARGS
        assert L.mag_get_refine_info(None, info) == MAG_ERR_BAD_ARGS
        assert L.mag_download_refine(None, C.byref(out)) == MAG_ERR_BAD_ARGS
        assert L.mag_upload_refined(None) == MAG_ERR_BAD_ARGS
        assert L.mag_run_refine(h, None) == MAG_ERR_BAD_ARGS and b"null options" in L.mag_last_error(h)
        for rule in (-1, 3, 99):
            assert L.mag_run_refine(h, C.byref(good(rule=rule))) == MAG_ERR_BAD_ARGS and b"mag_refine_rule" in L.mag_last_error(h)
        for split in (0, 2, 4, -1):
            assert L.mag_run_refine(h, C.byref(good(split=split))) == MAG_ERR_BAD_ARGS and b"split" in L.mag_last_error(h)
        for rule in (1, 2):
            for theta in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
                assert L.mag_run_refine(h, C.byref(good(rule=rule, theta=theta))) == MAG_ERR_BAD_ARGS and b"theta" in L.mag_last_error(h)
        assert L.mag_run_refine(h, C.byref(good(rule=0, theta=-1.0))) == MAG_ERR_STATE  # (theta is not read under rule 0)
        assert L.mag_run_refine(h, C.byref(good(marks=None))) == MAG_ERR_BAD_ARGS and b"null marks" in L.mag_last_error(h)
        for rule in (0, 1, 2):
            for split in (1, 3):
                assert L.mag_run_refine(h, C.byref(good(rule=rule, split=split, theta=1.0))) == MAG_ERR_STATE
                assert b"mag_run_refine before mag_upload" in L.mag_last_error(h)
        assert L.mag_get_refine_info(h, None) == MAG_ERR_BAD_ARGS and b"null info" in L.mag_last_error(h)
        assert L.mag_download_refine(h, None) == MAG_ERR_BAD_ARGS and b"null refined mesh" in L.mag_last_error(h)
        for call, name in ((lambda: L.mag_get_refine_info(h, info), b"mag_get_refine_info"), (lambda: L.mag_download_refine(h, C.byref(out)), b"mag_download_refine"),
                           (lambda: L.mag_upload_refined(h), b"mag_upload_refined")):
            assert call() == MAG_ERR_STATE and name + b" before a completed mag_run_refine" in L.mag_last_error(h)
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        for rule in (0, 1, 2):
            assert L.mag_run_refine(h, C.byref(good(rule=rule))) == MAG_ERR_BAD_ARGS and b"communicator" in L.mag_last_error(h)
    finally:
        L.mag_destroy(h)


def test_the_error_paths_in_a_compiled_caller(built, tmp_path):
    """tests/cpp/refine_errors.cpp: the same paths from C++, stand-alone (it is also what a host sanitizer build runs)."""
    exe = str(tmp_path / "refine_errors")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "refine_errors.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip", "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr


def test_python_mirror_names_the_rules_and_the_call_order(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        with pytest.raises(MagnetiteError, match="rule must be one of"):
            c.run_refine(rule="largest")
        for call in (lambda: c.run_refine(rule="top_fraction"), lambda: c.run_refine(rule="max_fraction", theta=0.5), c.refine_info, c.download_refine,
                     c.upload_refined, c.refine):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE
        with pytest.raises(MagnetiteError) as e:
            c.run_refine(rule="top_fraction", theta=0.0)
        assert e.value.code == MAG_ERR_BAD_ARGS
        with pytest.raises(MagnetiteError) as e:
            c.run_refine(rule="top_fraction", split=2)
        assert e.value.code == MAG_ERR_BAD_ARGS
