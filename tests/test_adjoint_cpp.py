"""include/magnetite_solver.hpp, solver::adjoint: compiles against the C ABI on any box and -- on the GPU box -- returns for the
tensile fixture, alone and in three materials, exactly the bits the Python binding returns."""
import os
import subprocess

import numpy as np
import pytest

import adjoint_ref as aref
from test_variants_cpp import sum_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_adjoint.cpp")
GOLD = os.path.join(ROOT, "tests", "golden")


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_adjoint_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_adjoint"))
    r = subprocess.run([str(tmp_path / "run_adjoint")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no input file" in r.stdout  # (before any library call)


def write_problem(path, prob, w):
    """The text form tests/cpp/run_adjoint.cpp reads, every double as a hexadecimal literal."""
    hx = lambda v: float(v).hex()
    with open(path, "w") as out:
        print(prob.mesh.num_nodes, prob.mesh.num_elements, hx(prob.youngs_modulus), hx(prob.poisson_ratio), hx(prob.part_thickness), file=out)
        for i, (x, y) in enumerate(prob.mesh.xy):
            print(hx(x), hx(y), int(prob.u_known[2 * i]), int(prob.u_known[2 * i + 1]), hx(prob.u_in[2 * i]), hx(prob.u_in[2 * i + 1]),
                  hx(prob.f_in[2 * i]), hx(prob.f_in[2 * i + 1]), file=out)
        for tri in prob.mesh.conn:
            print(*[int(n) for n in tri], file=out)
        for v in w:
            print(hx(v), file=out)


@pytest.mark.gpu
def test_cpp_adjoint_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    from test_member_sets_gpu import tensile
    prob = tensile()
    materials = np.array([[prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness], [110e9, 0.25, 0.75], [40e9, 0.38, 0.3]])
    got = {}
    with Context(device=0) as c:
        out = c.solve(prob)
        w = aref.patch_weights(prob)
        w *= out["rhs_norm"] / np.linalg.norm(aref.dJ1(w, out["u"])[prob.u_known == 0])
        got["run", 0] = c.adjoint(aref.dJ1(w, out["u"]), "run")[0]
        c.set_variants(material=materials)
        c.run_variants()
        G = np.stack([aref.dJ1(w, c.download_variant(i)[0]) for i in range(3)])
        for i, a in enumerate(c.adjoint(G, "variants")):
            got["variant", i] = a
    exe, data = str(tmp_path / "run_adjoint"), str(tmp_path / "tensile.txt")
    compile_to(exe)
    write_problem(data, prob, w)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    rows = {(ln.split()[0], int(ln.split()[1])): ln.split() for ln in r.stdout.splitlines() if ln.split()[0] in ("run", "variant")}
    assert sorted(rows) == sorted(got)
    for key, a in got.items():
        row = rows[key]
        want = [sum_in_order(v * v for v in a["lambda"]), sum_in_order(v * v for v in a["dloads"]), sum_in_order(a["delem"]),
                sum_in_order(v * v for v in a["dxy"])]
        assert [float.fromhex(v) for v in row[3:7]] == want, key
        assert [float.fromhex(v) for v in row[8:12]] == [a[k] for k in aref.SCALARS], key
        assert want[0] > 0 and want[3] > 0, key
