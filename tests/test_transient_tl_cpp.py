"""include/magnetite_solver.hpp, solver::transient_tl and solver::assemble_effective_tangent, and tools/magnetite_gpu.cpp
--transient ... --kinematics tl: both compile against the C ABI on any box and the tool's --dry-run parses the flags; on the GPU box
the C++ mirror returns for plate16 under a pull of 5 % exactly the bits the Python binding returns, and the tool on the beam prints a
line per step with its Newton and CG iterations and writes a history.csv that is the binding's run, digit for digit.

The tool's mesh reader turns every small element clockwise (the reference's check_ccw compares the area with 1.0) and
mag_run_transient_tl refuses such a mesh: the tool turns the elements back by their true sign, and so does the Python leg here."""
import os
import subprocess

import numpy as np
import pytest

import modal_ref
import transient_tl_cases as cases
from magnetite_amd.inputs import problem_from_input
from magnetite_amd.msh import parse_mesh
from test_cpp_driver import exe  # noqa: F401 (fixture)
from test_design_cpp import write_problem
from test_newton_cpp import beam_files  # noqa: F401 (fixture)
from test_variants_cpp import sum_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_transient_tl.cpp")
RHO = cases.RHO
INFO = ("steps", "cg_kernel", "preconditioner", "newton_iterations_total", "max_step_newton", "cg_iterations_total", "inverted", "converged")
RUN = ("steps", "cg_kernel", "preconditioner", "cg_iterations", "max_step_iterations", "snapshots_kept", "resumed", "converged")
DT = 2.0e-5


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_transient_tl_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_transient_tl"))


def test_the_tool_parses_the_flags_without_a_gpu(exe, beam_files):
    d = beam_files
    base = [exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run"]
    run = ["--transient", "16", "--dt", "2e-5", "--density", "2700"]
    r = subprocess.run(base + run + ["--kinematics", "tl", "--newton-tol", "1e-9", "--rayleigh", "0.5,0", "--probe", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dry-run: transient steps 16 dt 0.00002 density 2700 rayleigh 0.5,0 probes 1" in r.stdout, r.stdout
    assert "dry-run: transient kinematics total-lagrangian newton_tol 0.000000001" in r.stdout.splitlines(), r.stdout
    r = subprocess.run(base + run + ["--kinematics", "linear"], capture_output=True, text=True)
    assert r.returncode == 0 and "dry-run: transient kinematics linear newton_tol 0" in r.stdout.splitlines(), r.stdout + r.stderr
    r = subprocess.run(base + run, capture_output=True, text=True)
    assert r.returncode == 0 and "kinematics" not in r.stdout, r.stdout  # (without the flag nothing changes)
    r = subprocess.run(base + run + ["--kinematics", "tl", "--rayleigh", "0.5,1e-7"], capture_output=True, text=True)
    assert r.returncode == 1 and "--kinematics tl" in r.stderr and "--rayleigh A,0" in r.stderr and "--transient" in r.stderr, r.stderr
    r = subprocess.run(base + run + ["--newton-tol", "1e-9"], capture_output=True, text=True)  # (the linear pass has no Newton loop)
    assert r.returncode == 1 and "--newton-tol" in r.stderr, r.stderr
    r = subprocess.run(base + run + ["--kinematics", "tl", "--newton-tol", "-1"], capture_output=True, text=True)
    assert r.returncode == 1 and "--newton-tol" in r.stderr, r.stderr
    r = subprocess.run(base + run + ["--kinematics", "foo"], capture_output=True, text=True)
    assert r.returncode == 1 and "--kinematics foo" in r.stderr and "linear or tl" in r.stderr, r.stderr


@pytest.mark.gpu
def test_cpp_transient_tl_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    s = cases.setup("plate16", "pull5d")
    prob, alpha, u0, dt = s["prob"], s["alpha"], s["u0"], s["dt"]
    N = prob.mesh.num_nodes
    write_problem(tmp_path / "plate16.txt", prob)
    binary = str(tmp_path / "run_transient_tl")
    compile_to(binary)
    r = subprocess.run([binary, str(tmp_path / "plate16.txt"), float(dt).hex(), float(alpha).hex()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    with Context(device=0) as c:
        c.upload_problem(prob)
        got = c.transient(steps=6, dt=dt, density=RHO, rayleigh=(alpha, 0.0), u0=u0, energies=True, snapshot_every=2, probes=[3, N, 2 * N - 1],
                          kinematics="tl", newton_tol=1e-10, cg_tol=1e-12)
        run = c.transient_info()
        got["effective_tangent"] = c.assemble_effective_tangent(got["u"], 0.25 * dt * dt, 1.0, RHO)
    assert got["converged"] == 1 and got["newton_iterations"][1:].min() >= 2 and np.any(got["v"] != 0)
    assert [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "info"] == [[int(got[k]) for k in INFO]]
    assert [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "run"] == [[run[k] for k in RUN]]
    assert [[float.fromhex(v) for v in ln[1:]] for ln in lines if ln[0] == "time"] == [[got["t_start"], got["t_end"]]]
    sums = {ln[1]: float.fromhex(ln[2]) for ln in lines if ln[0] == "sum"}
    assert set(sums) == {"u", "v", "a", "f", "snapshots", "energies", "newton_residuals", "elements", "effective_tangent"}
    for k, v in sums.items():
        assert v == sum_in_order(got[k].reshape(-1)), k
    steps = [ln for ln in lines if ln[0] == "step"]
    assert len(steps) == 7
    for n, row in enumerate(steps):
        assert int(row[2]) == got["newton_iterations"][n] and int(row[3]) == got["iterations"][n], n
        want = [got[k][n, p] for p in range(3) for k in ("probe_u", "probe_v", "probe_a")]
        assert [float.fromhex(v) for v in row[4:]] == want, n


@pytest.mark.gpu
def test_the_tool_prints_the_steps_and_writes_the_history(exe, beam_files, tmp_path):
    from magnetite_amd import Context
    from magnetite_amd.post_processor import _fmt
    d = beam_files
    prob = problem_from_input(parse_mesh(str(d / "geom.msh")), str(d / "input.json"))
    N = prob.mesh.num_nodes
    tip = int(np.argmax(prob.mesh.xy[:, 0] + prob.mesh.xy[:, 1]))
    probes = [2 * tip, 2 * tip + 1, 2 * N - 1]
    r = subprocess.run([exe, str(d / "input.json"), str(d / "geom.msh"), "--nodes", str(tmp_path / "nodes.csv"), "--elements",
                        str(tmp_path / "elements.csv"), "--transient", "6", "--dt", repr(DT), "--density", "2700", "--kinematics", "tl",
                        "--newton-tol", "1e-9"] + [w for p in probes for w in ("--probe", str(p))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["elements.csv", "history.csv", "nodes.csv"]
    conn = np.array(prob.mesh.conn)
    clockwise = modal_ref.signed_areas(prob.mesh.xy, conn) < 0.0  # (the tool turns these back)
    conn[clockwise] = conn[clockwise][:, ::-1]
    with Context(device=0) as c:
        c.upload(prob.xy_flat, np.ascontiguousarray(conn), prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio,
                 prob.part_thickness)
        got = c.transient(steps=6, dt=DT, density=RHO, probes=probes, kinematics="tl", newton_tol=1e-9)
    assert got["converged"] == 1 and got["newton_iterations"][1:].min() >= 2
    out = r.stdout.splitlines()
    assert "info: transient kinematics total-lagrangian" in out and "warning: transient" not in r.stdout
    assert out.index("info: transient kinematics total-lagrangian") < min(i for i, ln in enumerate(out) if ln.startswith("info: step "))
    lines = [ln.split() for ln in out if ln.startswith("info: step ")]
    assert len(lines) == 7
    for n, ln in enumerate(lines):
        assert ln[2:] == [str(n), "t", _fmt(n * DT), "newton", str(got["newton_iterations"][n]), "iterations", str(got["iterations"][n])], ln
    text = (tmp_path / "history.csv").read_text().splitlines()
    assert text[0] == "step,t," + ",".join(f"u{p},v{p},a{p}" for p in probes) and len(text) == 8
    for n in range(7):  # the reference's float formatting, digit for digit
        want = [str(n), _fmt(n * DT)] + [_fmt(got[k][n, p]) for p in range(3) for k in ("probe_u", "probe_v", "probe_a")]
        assert text[1 + n].split(",") == want, n
