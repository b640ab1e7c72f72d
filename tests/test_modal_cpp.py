"""include/magnetite_solver.hpp, solver::modal, and tools/magnetite_gpu.cpp --modal: both compile against the C ABI on any box and
-- on the GPU box -- return for the tensile fixture exactly the bits the Python binding returns; the tool prints a line per mode
and writes modes.csv next to nodes.csv / elements.csv, which stay byte for byte what they are without the flag.

The fixture's elements are all clockwise (the reference's check_ccw compares the area with 1.0) and mag_run_modal refuses such a
mesh: the compiled caller gets the fixture with every element turned, and the tool turns them itself."""
import os
import subprocess

import numpy as np
import pytest

from magnetite_amd.inputs import problem_from_input
from magnetite_amd.msh import parse_mesh
from test_cpp_driver import exe, tensile_files  # noqa: F401 (fixtures)
from test_stress_recovery_cpp import MATERIAL, write_problem
from test_variants_cpp import sum_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "cpp", "run_modal.cpp")
RHO = 2700.0
INFO = ("modes", "subspace", "outer", "converged", "vectors_per_launch", "launches", "redone")


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def counter_clockwise(g):
    """the tensile fixture with every (clockwise) element turned"""
    turned = {k: g[k] for k in g.files}
    turned["conn"] = np.ascontiguousarray(g["conn"].reshape(-1, 3)[:, ::-1])
    return turned


def test_cpp_modal_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_modal"))


def test_the_tool_still_parses_without_a_gpu(exe, tensile_files):
    d, _ = tensile_files
    r = subprocess.run([exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run", "--modal", "4", "--density", "2700"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "dry-run:" in r.stdout, r.stderr
    r = subprocess.run([exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run", "--modal", "4"], capture_output=True, text=True)
    assert r.returncode == 1 and "--density" in r.stderr


@pytest.mark.gpu
def test_cpp_modal_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    g = counter_clockwise(np.load(os.path.join(GOLD, "tensile.npz")))
    write_problem(tmp_path / "tensile.txt", g)
    binary = str(tmp_path / "run_modal")
    compile_to(binary)
    r = subprocess.run([binary, str(tmp_path / "tensile.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    info = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "info"]
    modes = [ln for ln in lines if ln[0] == "mode"]
    with Context(device=0) as c:
        c.upload(g["xy"].reshape(-1), g["conn"].reshape(-1), g["u_known"], g["u_in"], g["f_in"], *MATERIAL)
        got = c.modal(modes=4, density=RHO)
    assert got["converged"] == 1 and np.all(got["lambda"] > 0)
    assert info == [[got[k] for k in INFO]]
    assert len(modes) == 4
    for k, row in enumerate(modes):
        assert [float.fromhex(v) for v in row[2:5]] == [got["lambda"][k], got["frequency"][k], got["residual"][k]], k
        assert float.fromhex(row[6]) == sum_in_order(got["shapes"][k]), k


@pytest.mark.gpu
def test_the_tool_writes_the_modes_and_leaves_the_other_files_as_they_are(exe, tensile_files, tmp_path):
    from magnetite_amd import Context
    from magnetite_amd.post_processor import _fmt
    d, g = tensile_files
    args = [exe, str(d / "input.json"), str(d / "geom.msh")]
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    outs = {}
    for where, extra in ((plain, []), (flagged, ["--modal", "4", "--density", "2700"])):
        where.mkdir()
        r = subprocess.run(args + ["--nodes", str(where / "nodes.csv"), "--elements", str(where / "elements.csv")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[where] = r.stdout
    assert sorted(os.listdir(plain)) == ["elements.csv", "nodes.csv"]
    assert "info: mode " not in outs[plain]
    assert sorted(os.listdir(flagged)) == ["elements.csv", "modes.csv", "nodes.csv"]
    for name in ("nodes.csv", "elements.csv"):
        assert (plain / name).read_bytes() == (flagged / name).read_bytes(), name
    prob = problem_from_input(parse_mesh(str(d / "geom.msh")), str(d / "input.json"))
    turned = np.ascontiguousarray(prob.mesh.conn[:, ::-1])  # (all clockwise after check_ccw: the tool turns every element)
    with Context(device=0) as c:
        c.upload(prob.xy_flat, turned, prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
        got = c.modal(modes=4, density=RHO)
    N = prob.mesh.num_nodes
    text = (flagged / "modes.csv").read_text().splitlines()
    assert text[0] == "id,ux1,uy1,ux2,uy2,ux3,uy3,ux4,uy4" and len(text) == N + 1
    for i in (0, 1, N // 2, N - 1):  # the reference's float formatting, digit for digit
        want = [str(i)] + [_fmt(got["shapes"][k, 2 * i + a]) for k in range(4) for a in (0, 1)]
        assert text[1 + i].split(",") == want, i
    rows = np.loadtxt(flagged / "modes.csv", delimiter=",", skiprows=1)
    assert np.array_equal(rows[:, 0], np.arange(N))
    assert np.array_equal(rows[:, 1:].reshape(N, 4, 2).transpose(1, 0, 2).reshape(4, 2 * N), got["shapes"])
    lines = [ln.split() for ln in outs[flagged].splitlines() if ln.startswith("info: mode ")]
    assert len(lines) == 4
    for k, ln in enumerate(lines):
        assert ln[2] == str(k + 1) and ln[3] == "frequency" and ln[5] == "Hz" and ln[6] == "residual"
        assert float(ln[4]) == got["frequency"][k] and float(ln[7]) == got["residual"][k]
