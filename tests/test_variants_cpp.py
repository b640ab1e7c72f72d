"""include/magnetite_solver.hpp, solver::run_variants: compiles against the C ABI on any box and -- on the GPU box -- returns for
three material variants of the patch-test mesh exactly the bits the Python binding returns."""
import os
import subprocess

import numpy as np
import pytest

from load_cases_util import patch_cases, patch_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_variants.cpp")
MATERIALS = np.array([[69e9, 0.33, 0.5], [110e9, 0.25, 0.75], [40e9, 0.38, 0.3]])


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_run_variants_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_variants"))


def sum_in_order(values):
    s = 0.0
    for v in values:  # the C++ program's left-to-right sums
        s += float(v)
    return s


@pytest.mark.gpu
def test_cpp_run_variants_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    exe = str(tmp_path / "run_variants")
    compile_to(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    info = [int(v) for v in lines[0].split()[1:]]
    rows = [ln.split() for ln in lines if ln.startswith("variant ")]
    xy, conn = patch_mesh()
    known, u, f = patch_cases()
    with Context(device=0) as c:
        c.upload(xy, conn, known, u[0], np.zeros_like(f[0]), 69e9, 0.33, 0.5)
        c.set_variants(material=MATERIALS)
        c.run_variants()
        assert list(c.variants_info().values()) == info and info[0] == 3 and info[1] >= 3 and info[2] == 1
        for i in range(3):
            pu, pf, ps = c.download_variant(i)
            assert c.variant_stats(i)["iterations"] == int(rows[i][3])
            su = sum_in_order(a + b for a, b in pu.reshape(-1, 2))
            sf = sum_in_order(a + b for a, b in pf.reshape(-1, 2))
            got = [float.fromhex(v) for v in rows[i][5:8]]
            assert got == [su, sf, sum_in_order(ps)], (i, got)
