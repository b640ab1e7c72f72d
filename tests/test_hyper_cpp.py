"""include/magnetite_solver.hpp, solver::set_material_law / solver::material_law, and tools/magnetite_gpu.cpp --material: the tool
compiles against the C ABI on any box and its --dry-run parses the flag and refuses it with the linear passes; on the GPU box
--material neo-hooke --nonlinear 4 on the strip squeezed to half its length prints "info: material neo-hooke" and four increment
lines, and writes a load_path.csv and a nodes.csv that are the Python binding's result under set_material_law("neo_hooke"), digit
for digit -- and not the St. Venant-Kirchhoff one, which does not converge there."""
import json
import subprocess

import numpy as np
import pytest

import hyper_ref as hr
import modal_ref
from magnetite_amd import meshgen
from magnetite_amd.inputs import problem_from_input
from magnetite_amd.msh import parse_mesh, write_msh
from test_cpp_driver import exe  # noqa: F401 (fixture)

EDGE = 1e-9
STRIP_JSON = {
    "metadata": {"part_thickness": 0.5, "material_elasticity": 69e9, "poisson_ratio": 0.33,
                 "characteristic_length_min": 0, "characteristic_length_max": 0.3},
    # (a later rule overrides an earlier one on both axes of a node: the corners get rules of their own)
    "boundary_conditions": {
        "left": {"region": {"x_target_max": EDGE}, "targets": {"ux": 0, "uy": None, "fx": None, "fy": 0}},
        "right": {"region": {"x_target_min": 1 - EDGE}, "targets": {"ux": -0.5, "uy": None, "fx": None, "fy": 0}},
        "bottom": {"region": {"x_target_min": EDGE, "x_target_max": 1 - EDGE, "y_target_max": EDGE},
                   "targets": {"ux": None, "uy": 0, "fx": 0, "fy": None}},
        "corner_left": {"region": {"x_target_max": EDGE, "y_target_max": EDGE}, "targets": {"ux": 0, "uy": 0, "fx": None, "fy": None}},
        "corner_right": {"region": {"x_target_min": 1 - EDGE, "y_target_max": EDGE}, "targets": {"ux": -0.5, "uy": 0, "fx": None, "fy": None}},
    },
}


@pytest.fixture(scope="module")
def strip_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip")
    write_msh(meshgen.plate(8, 4, lx=1.0, ly=0.5), str(d / "geom.msh"))
    (d / "input.json").write_text(json.dumps(STRIP_JSON))
    return d


def test_the_files_pose_the_twins_strip(strip_files):
    d = strip_files
    prob = problem_from_input(parse_mesh(str(d / "geom.msh")), str(d / "input.json"))
    want = hr.strip_problem()
    assert np.array_equal(prob.u_known, want.u_known) and np.array_equal(prob.u_in, want.u_in) and not prob.f_in.any()
    assert np.allclose(prob.mesh.xy, want.mesh.xy, rtol=0, atol=1e-15) and prob.poisson_ratio == want.poisson_ratio


def test_the_tool_parses_the_material_without_a_gpu(exe, strip_files):
    d = strip_files
    base = [exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run"]
    for flags in (["--nonlinear", "4"], ["--explicit", "8", "--density", "2700", "--kinematics", "tl"],
                  ["--transient", "8", "--dt", "1e-5", "--density", "2700", "--kinematics", "tl"]):
        for law in ("neo-hooke", "svk"):
            r = subprocess.run(base + flags + ["--material", law], capture_output=True, text=True)
            assert r.returncode == 0 and f"dry-run: material {law}" in r.stdout.splitlines(), r.stdout + r.stderr
        r = subprocess.run(base + flags, capture_output=True, text=True)
        assert r.returncode == 0 and "material" not in r.stdout  # (without the flag nothing changes)
    r = subprocess.run(base + ["--nonlinear", "4", "--material", "mooney"], capture_output=True, text=True)
    assert r.returncode == 1 and "--material mooney: svk or neo-hooke" in r.stderr, r.stderr
    for linear in ([], ["--explicit", "8", "--density", "2700"], ["--explicit", "8", "--density", "2700", "--kinematics", "linear"],
                   ["--transient", "8", "--dt", "1e-5", "--density", "2700"], ["--modal", "3", "--density", "2700"]):
        r = subprocess.run(base + linear + ["--material", "neo-hooke"], capture_output=True, text=True)
        assert r.returncode == 1 and "the linear passes read no material law" in r.stderr, (linear, r.stderr)


@pytest.mark.gpu
def test_the_tool_solves_the_strip_under_neo_hooke(exe, strip_files, tmp_path):
    from magnetite_amd import Context
    from magnetite_amd.post_processor import _fmt
    d = strip_files
    prob = problem_from_input(parse_mesh(str(d / "geom.msh")), str(d / "input.json"))
    N = prob.mesh.num_nodes
    top_right = int(np.argmax(prob.mesh.xy[:, 0] + prob.mesh.xy[:, 1]))
    probes = [2 * top_right, 2 * top_right + 1]
    r = subprocess.run([exe, str(d / "input.json"), str(d / "geom.msh"), "--nodes", str(tmp_path / "nodes.csv"), "--elements",
                        str(tmp_path / "elements.csv"), "--material", "neo-hooke", "--nonlinear", "4"] + [w for p in probes for w in ("--probe", str(p))],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "info: material neo-hooke" in r.stdout.splitlines() and "warning: nonlinear" not in r.stdout
    conn = np.array(prob.mesh.conn)
    clockwise = modal_ref.signed_areas(prob.mesh.xy, conn) < 0.0  # (the tool turns these back)
    conn[clockwise] = conn[clockwise][:, ::-1]
    with Context(device=0) as c:
        c.upload(prob.xy_flat, np.ascontiguousarray(conn), prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio,
                 prob.part_thickness)
        c.set_material_law("neo_hooke")
        got = c.newton(increments=4, probes=probes)
    want = hr.case_run("neo_hooke", "strip", "strip", 4)
    assert got["converged"] == 1 and got["inverted"] == 0 and list(got["newton_iterations"]) == list(want["newton_iterations"])
    lateral = got["u"][2 * top_right + 1] / 0.5 + 1.0
    print("the strip at stretch 0.5: lateral stretch", lateral, "iterations", got["newton_iterations"])
    assert abs(lateral - 1.23515) < 5e-6
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("info: increment ")]
    assert len(lines) == 4
    at = 0
    for k, ln in enumerate(lines, start=1):
        n = int(got["newton_iterations"][k])
        cg = int(got["cg_iterations"][at:at + n].sum())
        at += n
        assert ln[2:] == [str(k), "load", _fmt(k / 4), "newton", str(n), "cg", str(cg), "residual", _fmt(got["residuals"][at - 1])], ln
    text = (tmp_path / "load_path.csv").read_text().splitlines()
    assert len(text) == 6
    for k in range(5):  # the reference's float formatting, digit for digit
        row = [str(k), _fmt(got["load"][k]), str(got["newton_iterations"][k]), _fmt(got["energies"][k, 0]), _fmt(got["energies"][k, 1])] + \
            [_fmt(v) for v in got["probe_u"][k]]
        assert text[1 + k].split(",") == row, k
    nodes = (tmp_path / "nodes.csv").read_text().splitlines()
    assert len(nodes) == N + 1
    for i in (0, top_right, N - 1):
        assert nodes[1 + i].split(",")[2:] == [_fmt(got["u"][2 * i]), _fmt(got["u"][2 * i + 1])], i
