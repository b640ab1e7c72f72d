"""include/magnetite_solver.hpp, solver::run_explicit with kinematics = MAG_KIN_TOTAL_LAGRANGIAN and solver::internal_force, and
tools/magnetite_gpu.cpp --explicit ... --kinematics: both compile against the C ABI on any box; the tool's --dry-run parses the
flag; on the GPU box the C++ mirror returns for plate16 under a pull of 5 % exactly the bits the Python binding returns."""
import os
import subprocess

import numpy as np
import pytest

import explicit_tl_cases as cases
from test_cpp_driver import exe  # noqa: F401 (fixture)
from test_design_cpp import write_problem
from test_explicit_cpp import plate_files  # noqa: F401 (fixture)
from test_variants_cpp import sum_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_explicit_tl.cpp")
RHO = cases.RHO
INFO = ("steps", "method", "fused", "step_launches", "record_every", "snapshots_kept", "resumed")


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_explicit_tl_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_explicit_tl"))


def test_the_tool_parses_the_kinematics_without_a_gpu(exe, plate_files):
    d = plate_files
    base = [exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run"]
    explicit = ["--explicit", "64", "--density", "2700"]
    r = subprocess.run(base + explicit + ["--kinematics", "tl", "--rayleigh", "0.5,0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dry-run: explicit steps 64 dt 0 dt_scale 0 density 2700 rayleigh 0.5,0 probes 0 record_every 1" in r.stdout, r.stdout
    assert "dry-run: explicit kinematics total-lagrangian" in r.stdout.splitlines(), r.stdout
    r = subprocess.run(base + explicit + ["--kinematics", "linear", "--rayleigh", "0.5,1e-7"], capture_output=True, text=True)
    assert r.returncode == 0 and "dry-run: explicit kinematics linear" in r.stdout.splitlines(), r.stdout + r.stderr
    r = subprocess.run(base + explicit, capture_output=True, text=True)
    assert r.returncode == 0 and "kinematics" not in r.stdout, r.stdout  # (without the flag nothing changes)
    r = subprocess.run(base + explicit + ["--kinematics", "foo"], capture_output=True, text=True)
    assert r.returncode == 1 and "--kinematics foo" in r.stderr and "linear or tl" in r.stderr, r.stderr
    r = subprocess.run(base + explicit + ["--kinematics", "tl", "--rayleigh", "0.5,1e-7"], capture_output=True, text=True)
    assert r.returncode == 1 and "--kinematics tl" in r.stderr and "--rayleigh A,0" in r.stderr, r.stderr
    r = subprocess.run(base + ["--kinematics", "tl"], capture_output=True, text=True)
    assert r.returncode == 1 and "--explicit" in r.stderr, r.stderr


@pytest.mark.gpu
def test_cpp_explicit_tl_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    s = cases.setup("plate16", "pull5")
    prob, alpha, u0 = s["prob"], s["alpha"], s["u0"]
    N = prob.mesh.num_nodes
    write_problem(tmp_path / "plate16.txt", prob)
    binary = str(tmp_path / "run_explicit_tl")
    compile_to(binary)
    r = subprocess.run([binary, str(tmp_path / "plate16.txt"), float(alpha).hex()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    with Context(device=0) as c:
        c.upload_problem(prob)
        got = c.explicit(steps=40, density=RHO, rayleigh=(alpha, 0.0), u0=u0, energies=True, record_every=4, snapshot_every=8,
                         probes=[3, N, 2 * N - 1], kinematics="tl")
        got["f_int"], W, inverted = c.internal_force(u0)
    assert got["fused"] == 1 and got["method"] == 7 and np.any(got["v"] != 0) and not inverted and not got["inverted"]
    assert [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "info"] == [[got[k] for k in INFO]]
    assert [[float.fromhex(v) for v in ln[1:]] for ln in lines if ln[0] == "time"] == [[got["t_start"], got["t_end"], got["dt"], got["dt_bound"]]]
    assert [float.fromhex(ln[1]) for ln in lines if ln[0] == "energy"] == [W]
    sums = {ln[1]: float.fromhex(ln[2]) for ln in lines if ln[0] == "sum"}
    assert set(sums) == {"u", "v", "a", "f", "snapshots", "energies", "time", "f_int"}
    for k, v in sums.items():
        assert v == sum_in_order(got[k].reshape(-1)), k
    rows = [ln for ln in lines if ln[0] == "row"]
    assert len(rows) == 11
    for n, row in enumerate(rows):
        want = [got[k][n, p] for p in range(3) for k in ("probe_u", "probe_v", "probe_a")]
        assert [float.fromhex(v) for v in row[2:]] == want, n
