"""include/magnetite_solver.hpp, solver::run_newton and solver::assemble_tangent, and tools/magnetite_gpu.cpp --nonlinear: the tool
compiles against the C ABI on any box and its --dry-run parses the flags; on the GPU box --nonlinear 8 on the beam prints eight
increment lines and writes a load_path.csv whose last row is the Python binding's result, digit for digit, and nodes.csv /
elements.csv from the nonlinear state.

The tool's mesh reader turns every small element clockwise (the reference's check_ccw compares the area with 1.0) and
mag_run_newton refuses such a mesh: the tool turns the elements back by their true sign, and so does the Python leg here."""
import json
import os
import subprocess

import numpy as np
import pytest

import modal_ref
from magnetite_amd import meshgen
from magnetite_amd.inputs import problem_from_input
from magnetite_amd.msh import parse_mesh, write_msh
from test_cpp_driver import exe  # noqa: F401 (fixture)

BEAM_JSON = {
    "metadata": {"part_thickness": 0.5, "material_elasticity": 69e9, "poisson_ratio": 0.33,
                 "characteristic_length_min": 0, "characteristic_length_max": 0.3},
    "boundary_conditions": {
        "restraint": {"region": {"x_target_min": -1, "x_target_max": 1e-9}, "targets": {"ux": 0, "uy": 0, "fx": None, "fy": None}},
        "load": {"region": {"x_target_min": 1 - 1e-9, "x_target_max": 2}, "targets": {"ux": None, "uy": None, "fx": 0, "fy": -1.2e6}},
    },
}


@pytest.fixture(scope="module")
def beam_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("beam")
    write_msh(meshgen.plate(32, 4, lx=1.0, ly=0.125), str(d / "geom.msh"))
    (d / "input.json").write_text(json.dumps(BEAM_JSON))
    return d


def test_the_tool_parses_the_flags_without_a_gpu(exe, beam_files):
    d = beam_files
    base = [exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run"]
    r = subprocess.run(base + ["--nonlinear", "8", "--newton-tol", "1e-9", "--line-search", "4", "--probe", "3", "--probe", "8"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "dry-run: nodes 165 elements 256" in r.stdout, r.stdout + r.stderr
    assert "dry-run: nonlinear increments 8 newton_tol 0.000000001 line_search 4 probes 2" in r.stdout.splitlines(), r.stdout
    r = subprocess.run(base + ["--nonlinear", "2"], capture_output=True, text=True)
    assert r.returncode == 0 and "dry-run: nonlinear increments 2 newton_tol 0 line_search 0 probes 0" in r.stdout.splitlines(), r.stdout
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0 and "nonlinear" not in r.stdout  # (without the flag nothing changes)
    for wrong in (["--nonlinear", "0"], ["--nonlinear", "2", "--newton-tol", "-1"], ["--nonlinear", "2", "--line-search", "-1"],
                  ["--newton-tol", "1e-8"], ["--line-search", "2"]):
        r = subprocess.run(base + wrong, capture_output=True, text=True)
        assert r.returncode == 1 and "--nonlinear INCREMENTS" in r.stderr, (wrong, r.stderr)
    r = subprocess.run(base + ["--nonlinear", "2", "--transient", "4", "--dt", "1e-6", "--density", "2700"], capture_output=True, text=True)
    assert r.returncode == 1 and "one of them at a time" in r.stderr
    r = subprocess.run(base + ["--probe", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "--probe" in r.stderr  # (a probe still needs a pass that records it)


@pytest.mark.gpu
def test_the_tool_writes_the_load_path_and_the_nonlinear_state(exe, beam_files, tmp_path):
    from magnetite_amd import Context
    from magnetite_amd.post_processor import _fmt
    d = beam_files
    prob = problem_from_input(parse_mesh(str(d / "geom.msh")), str(d / "input.json"))
    N = prob.mesh.num_nodes
    tip = int(np.argmax(prob.mesh.xy[:, 0] + prob.mesh.xy[:, 1]))
    probes = [2 * tip, 2 * tip + 1, 2 * N - 1]
    r = subprocess.run([exe, str(d / "input.json"), str(d / "geom.msh"), "--nodes", str(tmp_path / "nodes.csv"), "--elements",
                        str(tmp_path / "elements.csv"), "--nonlinear", "8"] + [w for p in probes for w in ("--probe", str(p))],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["elements.csv", "load_path.csv", "nodes.csv"]
    conn = np.array(prob.mesh.conn)
    clockwise = modal_ref.signed_areas(prob.mesh.xy, conn) < 0.0  # (the tool turns these back)
    conn[clockwise] = conn[clockwise][:, ::-1]
    with Context(device=0) as c:
        c.upload(prob.xy_flat, np.ascontiguousarray(conn), prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio,
                 prob.part_thickness)
        got = c.newton(increments=8, probes=probes)
    assert got["converged"] == 1 and 0.2 < -got["u"][2 * tip + 1] < 0.3  # (the tip comes down a quarter of the length)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("info: increment ")]
    assert len(lines) == 8 and "warning: nonlinear" not in r.stdout
    at = 0
    for k, ln in enumerate(lines, start=1):
        n = int(got["newton_iterations"][k])
        cg = int(got["cg_iterations"][at:at + n].sum())
        at += n
        assert ln[2:] == [str(k), "load", _fmt(k / 8), "newton", str(n), "cg", str(cg), "residual", _fmt(got["residuals"][at - 1])], ln
    text = (tmp_path / "load_path.csv").read_text().splitlines()
    assert text[0] == "increment,load,newton,W,Pi," + ",".join(f"u{p}" for p in probes) and len(text) == 10
    for k in range(9):  # the reference's float formatting, digit for digit
        want = [str(k), _fmt(got["load"][k]), str(got["newton_iterations"][k]), _fmt(got["energies"][k, 0]), _fmt(got["energies"][k, 1])] + \
            [_fmt(v) for v in got["probe_u"][k]]
        assert text[1 + k].split(",") == want, k
    assert text[-1].split(",")[5:] == [_fmt(got["u"][p]) for p in probes]
    nodes = (tmp_path / "nodes.csv").read_text().splitlines()
    assert nodes[0] == "x,y,ux,uy" and len(nodes) == N + 1
    for i in (0, tip, N - 1):
        assert nodes[1 + i].split(",")[2:] == [_fmt(got["u"][2 * i]), _fmt(got["u"][2 * i + 1])], i
    sx, sy, sxy = got["elem"][:, 3], got["elem"][:, 4], got["elem"][:, 5]
    vm = np.sqrt(sx * sx - sx * sy + sy * sy + 3.0 * sxy * sxy)
    elems = (tmp_path / "elements.csv").read_text().splitlines()
    assert len(elems) == prob.mesh.num_elements + 1
    assert np.allclose([float(ln.split(",")[3]) for ln in elems[1:]], vm, rtol=1e-14, atol=0.0)
