"""include/magnetite_solver.hpp, solver::objective: compiles against the C ABI on any box and -- on the GPU box -- returns for the
tensile fixture, alone and in three materials, with the adjoint, exactly the bits the Python binding returns."""
import os
import subprocess

import numpy as np
import pytest

import adjoint_ref as aref
import objective_ref as oref
from test_adjoint_cpp import write_problem
from test_variants_cpp import sum_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_objective.cpp")
SCALARS = ("J", "pJ_pE", "pJ_pnu", "pJ_pt", "dJ_dE", "dJ_dnu", "dJ_dt")


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_cpp_objective_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_objective"))
    r = subprocess.run([str(tmp_path / "run_objective")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no input file" in r.stdout  # (before any library call)


@pytest.mark.gpu
def test_cpp_objective_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    from test_member_sets_gpu import tensile
    prob = tensile()
    materials = np.array([[prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness], [110e9, 0.25, 0.75], [40e9, 0.38, 0.3]])
    rng = np.random.default_rng(3)
    free = prob.u_known == 0
    got = {}
    with Context(device=0) as c:
        out = c.solve(prob)
        u = out["u"]
        sig = oref.element_stress(np.asarray(prob.mesh.xy).reshape(-1, 2), np.asarray(prob.mesh.conn).reshape(-1, 3), u, prob.poisson_ratio, prob.youngs_modulus)
        specs = {"stress_pnorm": dict(weights=rng.uniform(0.5, 1.5, prob.mesh.num_elements), p=6.0,
                                      scale=float(np.sqrt(oref.von_mises_sq(sig)).max())),
                 "disp_lsq": dict(weights=aref.patch_weights(prob), target=0.5 * u)}
        for kind, spec in specs.items():  # |g_F| of the size of the right-hand side (g grows with w^(1/p) for the p-norm)
            g = c.objective(kind, "run", **spec)[0]["g"]
            spec["weights"] = spec["weights"] * (out["rhs_norm"] / np.linalg.norm(g[free])) ** spec.get("p", 1.0)
            got[kind, "run", 0] = c.objective(kind, "run", adjoint=True, **spec)[0]
        c.set_variants(material=materials)
        c.run_variants()
        for kind, spec in specs.items():
            for i, o in enumerate(c.objective(kind, "variants", adjoint=True, **spec)):
                got[kind, "variant", i] = o
    exe, data = str(tmp_path / "run_objective"), str(tmp_path / "tensile.txt")
    compile_to(exe)
    write_problem(data, prob, [])
    with open(data, "a") as f:
        print(float(specs["stress_pnorm"]["p"]).hex(), float(specs["stress_pnorm"]["scale"]).hex(), file=f)
        for v in np.concatenate([specs["stress_pnorm"]["weights"], specs["disp_lsq"]["weights"], specs["disp_lsq"]["target"]]):
            print(float(v).hex(), file=f)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    rows = {(ln.split()[0], ln.split()[1], int(ln.split()[2])): ln.split() for ln in r.stdout.splitlines() if ln.split()[0] in specs}
    assert sorted(rows) == sorted(got)
    for key, o in got.items():
        row = rows[key]
        want = [sum_in_order(v * v for v in o[k]) for k in ("g", "pxy", "dxy")]
        assert [float.fromhex(v) for v in row[4:7]] == want, key
        assert [float.fromhex(v) for v in row[8:15]] == [o[k] for k in SCALARS], key
        assert want[0] > 0 and want[2] > 0 and o["J"] > 0, key
