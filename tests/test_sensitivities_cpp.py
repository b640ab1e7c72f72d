"""include/magnetite_solver.hpp, solver::sensitivities: compiles against the C ABI on any box and -- on the GPU box -- returns for
the patch-test mesh, alone and in three materials, exactly the bits the Python binding returns."""
import os
import subprocess

import numpy as np
import pytest

from load_cases_util import patch_cases, patch_mesh
from test_variants_cpp import MATERIALS, sum_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_sensitivities.cpp")
SCALARS = ("strain_energy", "potential_energy", "external_work", "reaction_work", "dPi_dE", "dPi_dnu", "dPi_dt")


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_sensitivities_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_sensitivities"))


@pytest.mark.gpu
def test_cpp_sensitivities_equal_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    exe = str(tmp_path / "run_sensitivities")
    compile_to(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    rows = {(ln.split()[0], int(ln.split()[1])): ln.split() for ln in r.stdout.splitlines() if ln.split()[0] in ("run", "variant")}
    xy, conn = patch_mesh()
    known, u, f = patch_cases()
    with Context(device=0) as c:
        c.upload(xy, conn, known, u[0], f[1], 69e9, 0.33, 0.5)
        c.run()
        got = {("run", 0): c.sensitivities("run")[0]}
        c.set_variants(material=MATERIALS)
        c.run_variants()
        for i, s in enumerate(c.sensitivities("variants")):
            got[("variant", i)] = s
    assert sorted(rows) == sorted(got)
    for key, s in got.items():
        row = rows[key]
        sums = [float.fromhex(v) for v in row[3:5]]
        assert sums == [sum_in_order(s["energy"]), sum_in_order(v * v for v in s["dxy"])], key
        assert [float.fromhex(v) for v in row[6:13]] == [s[k] for k in SCALARS], key
    assert got[("run", 0)]["external_work"] != 0.0 and got[("run", 0)]["reaction_work"] != 0.0
