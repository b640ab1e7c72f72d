"""include/magnetite_solver.hpp, solver::run_cases: compiles against the C ABI on any box and -- on the GPU box -- returns for
two load sets on the patch-test mesh exactly the bits the Python binding returns."""
import os
import subprocess

import numpy as np
import pytest

from load_cases_util import patch_cases, patch_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_cases.cpp")


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_run_cases_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_cases"))


@pytest.mark.gpu
def test_cpp_run_cases_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    exe = str(tmp_path / "run_cases")
    compile_to(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    info = [int(v) for v in lines[0].split()[1:]]
    nodes = [[[float.fromhex(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("n ")]]
    nodes = np.array(nodes[0]).reshape(2, -1, 4)
    stress = np.array([float.fromhex(ln.split()[1]) for ln in lines if ln.startswith("s ")]).reshape(2, -1)
    its = [int(ln.split()[3]) for ln in lines if ln.startswith("case ")]
    xy, conn = patch_mesh()
    known, u, f = patch_cases()
    with Context(device=0) as c:
        c.upload(xy, conn, known, u[0], f[0], 69e9, 0.33, 0.5)
        c.set_load_cases(u, f)
        c.run_cases()
        assert list(c.cases_info().values()) == info and info[0] == 2 and info[1] >= 2 and info[2] == 1
        for i in range(2):
            pu, pf, ps = c.download_case(i)
            assert c.case_stats(i)["iterations"] == its[i]
            assert np.array_equal(pu.reshape(-1, 2), nodes[i][:, 0:2])
            assert np.array_equal(pf.reshape(-1, 2), nodes[i][:, 2:4])
            assert np.array_equal(ps, stress[i])
