"""include/magnetite_solver.hpp, solver::refine and solver::upload_refined, and tools/magnetite_gpu.cpp --adapt: both compile
against the C ABI on any box and -- on the GPU box -- return for the tensile fixture exactly the bits the Python binding returns;
the tool prints a line per solve of the loop and writes the final mesh, and without the flag its outputs stay byte for byte what
they are."""
import math
import os
import subprocess

import numpy as np
import pytest

from magnetite_amd.inputs import problem_from_input
from magnetite_amd.msh import parse_mesh
from test_cpp_driver import exe, tensile_files  # noqa: F401 (fixtures)
from test_stress_recovery_cpp import MATERIAL, write_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "cpp", "run_refine.cpp")
ARRAYS = dict(xy=np.float64, conn=np.int32, u_known=np.uint8, u_in=np.float64, f_in=np.float64, node_parents=np.int32, elem_parent=np.int32)


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_refine_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_refine"))


def test_the_tool_parses_the_flags_without_a_gpu(exe, tensile_files):
    d, _ = tensile_files
    args = [exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run"]
    plain = subprocess.run(args, capture_output=True, text=True)
    for extra in (["--adapt", "2"], ["--adapt", "2", "--refine-fraction", "0.3", "--refine-split", "3"]):
        r = subprocess.run(args + extra, capture_output=True, text=True)
        assert r.returncode == 0 and "dry-run:" in r.stdout, r.stderr
        assert r.stdout == plain.stdout
    for extra in (["--adapt", "-1"], ["--adapt", "2", "--refine-split", "2"], ["--adapt", "2", "--refine-fraction", "0"], ["--adapt", "1", "--refine-fraction", "1.5"]):
        r = subprocess.run(args + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "Input error" in r.stderr, (extra, r.stdout, r.stderr)


@pytest.mark.gpu
def test_cpp_refine_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    g = np.load(os.path.join(GOLD, "tensile.npz"))
    write_problem(tmp_path / "tensile.txt", g)
    binary = str(tmp_path / "run_refine")
    compile_to(binary)
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([binary, str(tmp_path / "tensile.txt"), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    rows = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines() if ln.split()[0] in ("top1", "max3", "marks1")}
    E = len(g["conn"].reshape(-1, 3))
    marks = np.zeros(E, dtype=np.uint8)
    marks[::7] = 1
    got = {}
    with Context(device=0) as c:
        c.upload(g["xy"].reshape(-1), g["conn"].reshape(-1), g["u_known"], g["u_in"], g["f_in"], *MATERIAL)
        got["marks1"] = c.refine(marks=marks)
        c.run()
        c.run_stress("run")
        got["top1"] = c.refine()
        got["max3"] = c.refine(rule="max_fraction", theta=0.5, split=3)
    assert sorted(rows) == sorted(got)
    for tag, m in got.items():
        for k, dtype in ARRAYS.items():
            assert np.fromfile(out / f"{tag}_{k}.bin", dtype=dtype).tobytes() == m[k].tobytes(), (tag, k)
        words = [int(v) for v in (rows[tag][2], rows[tag][4], rows[tag][6], rows[tag][8], rows[tag][10], *rows[tag][12:15])]
        assert words == [m[k] for k in ("nodes", "elements", "marked", "marked_edges", "sweeps", "split2", "split3", "split4")], tag
    assert got["top1"]["marked"] == math.ceil(0.2 * E) and got["max3"]["split4"] >= got["max3"]["marked"] >= 1
    # the adaptive loop: the binding's, line by line and array by array
    from magnetite_amd.meshgen import Mesh, Problem
    prob = Problem(Mesh(g["xy"].reshape(-1, 2), g["conn"].reshape(-1, 3)), g["u_known"], g["u_in"], g["f_in"], *MATERIAL)
    with Context(device=0) as c:
        want = c.adapt(prob, rounds=2)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("adapt ")]
    assert len(lines) == 3
    for ln, h in zip(lines, want["history"]):
        assert (int(ln[3]), int(ln[5]), float.fromhex(ln[7]), float.fromhex(ln[9]), int(ln[11])) == (h["nodes"], h["elements"], h["eta"], h["eta_rel"], h["iterations"])
    final = want["problem"]
    for k, a in dict(xy=final.mesh.xy, conn=final.mesh.conn, u_known=final.u_known, u_in=final.u_in, f_in=final.f_in).items():
        assert np.fromfile(out / f"adapt2_{k}.bin", dtype=ARRAYS[k]).tobytes() == np.ascontiguousarray(a).tobytes(), k
    assert np.fromfile(out / "adapt2_u.bin").tobytes() == want["result"]["u"].tobytes()


@pytest.mark.gpu
def test_the_tool_adapts_and_leaves_the_plain_outputs_as_they_are(exe, tensile_files, tmp_path):
    from magnetite_amd import Context
    from magnetite_amd.post_processor import csv_output_arrays
    d, g = tensile_files
    args = [exe, str(d / "input.json"), str(d / "geom.msh")]
    plain, adapted = tmp_path / "plain", tmp_path / "adapted"
    outs = {}
    for where, extra in ((plain, []), (adapted, ["--adapt", "2"])):
        where.mkdir()
        r = subprocess.run(args + ["--nodes", str(where / "nodes.csv"), "--elements", str(where / "elements.csv")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[where] = r.stdout
    # without the flag: the two files only, what the Python path writes for the same solve; nothing about the loop printed
    assert sorted(os.listdir(plain)) == ["elements.csv", "nodes.csv"] and "info: adapt round" not in outs[plain]
    prob = problem_from_input(parse_mesh(str(d / "geom.msh")), str(d / "input.json"))
    with Context(device=0) as c:
        out = c.solve(prob)
        csv_output_arrays(prob.xy_flat, prob.conn_flat, out["u"], out["stress"], str(tmp_path / "nodes.csv"), str(tmp_path / "elements.csv"))
        want = c.adapt(prob, rounds=2)
    for name in ("nodes.csv", "elements.csv"):
        assert (plain / name).read_bytes() == (tmp_path / name).read_bytes(), name
    # with it: a line per solve, the binding's numbers digit for digit, and the final mesh with its solution
    lines = [ln for ln in outs[adapted].splitlines() if ln.startswith("info: adapt round ")]
    assert len(lines) == 3, outs[adapted][-2000:]
    for r, (ln, h) in enumerate(zip(lines, want["history"])):
        w = ln.replace(",", "").replace(":", "").split()
        assert (int(w[3]), int(w[4]), int(w[6]), float(w[9])) == (r, h["nodes"], h["elements"], h["eta_rel"]), ln
    assert sorted(os.listdir(adapted)) == ["elements.csv", "nodes.csv"]
    nodes = np.loadtxt(adapted / "nodes.csv", delimiter=",", skiprows=1)
    els = np.loadtxt(adapted / "elements.csv", delimiter=",", skiprows=1)
    final = want["problem"]
    assert nodes.shape == (want["history"][-1]["nodes"], 4) and els.shape == (want["history"][-1]["elements"], 4)
    assert np.array_equal(nodes[:, :2], final.mesh.xy) and np.array_equal(els[:, :3], final.mesh.conn)
    assert np.array_equal(nodes[:, 2:].reshape(-1), want["result"]["u"]) and np.array_equal(els[:, 3], want["result"]["stress"])
    assert want["history"][-1]["elements"] > want["history"][0]["elements"]
