"""mag_options.field_cg through include/magnetite_solver.hpp (the C++ mirror passes mag_options itself): a compiled caller sets
the option, solves plate(6, 5) under a field, sees cg_kernel 5 and the solution of a field_cg = 0 run within the solve's bar."""
import os
import subprocess

import numpy as np
import pytest

import field_cg_ref as fref
from test_cpp_driver import exe, tensile_files  # noqa: F401 (fixtures)
from test_design_cpp import write_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_field_cg.cpp")


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_field_cg_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_field_cg"))


def test_the_tool_parses_field_cg_without_a_gpu(exe, tensile_files):
    d, _ = tensile_files
    args = [exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run"]
    plain = subprocess.run(args, capture_output=True, text=True)
    for k in ("0", "1", "2", "3"):
        r = subprocess.run(args + ["--topopt", "3", "--field-cg", k], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == plain.stdout, (k, r.stderr)
    for extra in (["--topopt", "3", "--field-cg", "4"], ["--topopt", "3", "--field-cg", "-1"], ["--field-cg", "2"]):
        r = subprocess.run(args + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "Input error" in r.stderr and "--field-cg" in r.stderr, (extra, r.stdout, r.stderr)


@pytest.mark.gpu
def test_cpp_sets_the_option_and_runs_the_block_rows(built, tmp_path):
    name, bc, which = "plate_6x5", "pull", "random"
    prob, sol, s = fref.problem(name, bc), fref.direct(name, bc, which), fref.field(name, which)
    write_problem(tmp_path / "plate.txt", prob)
    with open(tmp_path / "plate.txt", "a") as fh:
        fh.write("\n".join(float(v).hex() for v in s) + "\n")
    binary = str(tmp_path / "run_field_cg")
    compile_to(binary)
    r = subprocess.run([binary, str(tmp_path / "plate.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    runs = {int(ln[1]): int(ln[2]) for ln in lines if ln[0] == "run"}
    assert runs == {0: 3, 1: 5, 2: 5, 3: 5}
    u = {k: np.zeros(2 * prob.mesh.num_nodes) for k in runs}
    for ln in lines:
        if ln[0] == "u":
            u[int(ln[1])][2 * int(ln[2]):2 * int(ln[2]) + 2] = [float.fromhex(ln[3]), float.fromhex(ln[4])]
    bar = sol["cond"] * 10 * 1e-12  # the solve's bar on u in rel-L2: cond(K_ff) 10 tol
    for k in (1, 2, 3):
        assert np.linalg.norm(u[k] - u[0]) <= bar * np.linalg.norm(u[0]), k
        assert np.linalg.norm(u[k] - sol["u"]) <= bar * np.linalg.norm(sol["u"]), k
