"""sym_pencil_eig of csrc/modal_host.h (the Rayleigh-Ritz step of mag_run_buckling) through the stand-alone program
tests/cpp/pencil_eig.cpp, built and run as tests/test_modal.py does modal_eig.cpp; include/magnetite_solver.hpp, solver::buckling,
solver::apply_geometric and solver::assemble_geometric, and tools/magnetite_gpu.cpp --buckling: both compile against the C ABI on
any box and -- on the GPU box -- return for column8 of tests/buckling_ref.py exactly the bits the Python binding returns; the tool
prints a line per mode and writes buckling_modes.csv next to nodes.csv / elements.csv, which stay byte for byte what they are
without the flag."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import buckling_ref as ref
from test_cpp_driver import exe, tensile_files  # noqa: F401 (fixtures)
from test_modal import _sanitizer_flags
from test_variants_cpp import sum_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_buckling.cpp")
INFO = ("modes", "subspace", "outer", "converged", "vectors_per_launch", "launches", "redone", "positive")


def _parse(text):
    """[(n, status, pivot, dict(A, B, exact, least, mu, Q))] of pencil_eig's output"""
    pairs = []
    for line in text.splitlines():
        word, *rest = line.split()
        if word == "pair":
            pairs.append((int(rest[0]), int(rest[2]), int(rest[4]), {}))
        else:
            pairs[-1][3][word] = np.array([float.fromhex(t) for t in rest])
    return pairs


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_pencils_ritz_step_on_the_host(tmp_path):
    binary = tmp_path / "pencil_eig"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *_sanitizer_flags(tmp_path), "-I", os.path.join(ROOT, "magnetite_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "pencil_eig.cpp"), "-o", str(binary)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    first = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    assert first.returncode == 0, (first.stdout[-500:], first.stderr[-3000:])
    again = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    assert again.stdout == first.stdout  # the same input: the same bits
    pairs = _parse(first.stdout)
    assert [p[0] for p in pairs] == [1, 2, 14, 32, 3, 2]
    for n, status, pivot, m in pairs[:4]:
        assert status == 0
        A, B, mu, Q, exact = m["A"].reshape(n, n), m["B"].reshape(n, n), m["mu"], m["Q"].reshape(n, n), m["exact"]
        ortho = np.max(np.abs(Q.T @ A @ Q - np.eye(n)))
        diag = np.max(np.abs(Q.T @ B @ Q - np.diag(mu)))
        # the known mu by magnitude; where two magnitudes are equal (the +- pair, the zeros) either order is a right answer
        want = exact[np.argsort(-np.abs(exact), kind="stable")]
        err = max(np.max(np.abs(np.abs(mu) - np.abs(want))), np.max(np.abs(np.sort(mu) - np.sort(exact))))
        print("n", n, "|Q^T A Q - I|", ortho, "|Q^T B Q - diag(mu)|", diag, "mu error", err, "least pivot", m["least"][0])
        assert ortho <= 1e-12
        assert diag <= 1e-12
        assert err <= 1e-12
        assert np.all(np.diff(np.abs(mu)) <= 0)  # by |mu| descending
        big = np.abs(mu) > 1e-13  # (a zero mu comes out as a rounding error of either sign)
        assert (mu[big] > 0).sum() == (exact > 0).sum() and (mu[big] < 0).sum() == (exact < 0).sum()  # both signs stay
        assert 0 < m["least"][0] <= 1.0
        for k in range(n):  # the sign convention: sym_def_eig's
            assert Q[int(np.argmax(np.abs(Q[:, k]))), k] > 0
    n, status, pivot, m = pairs[1]
    assert np.max(np.abs(np.sort(m["mu"]) - [-0.5, 0.5])) <= 1e-12  # the +- pair: both of it
    assert np.min(np.abs(pairs[2][3]["mu"])) <= 1e-14 and np.sort(np.abs(pairs[3][3]["mu"]))[1] <= 1e-14  # the zero mu: n eps of the largest
    n, status, pivot, m = pairs[4]
    assert status == 2 and pivot == 2 and "mu" not in m and m["least"][0] <= 1e-13  # the rank-deficient A: refused, the column named
    n, status, pivot, m = pairs[5]
    assert status == 2 and pivot == 1 and "mu" not in m and m["least"][0] == 0.0  # a diagonal entry that is not positive


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def write_problem(path, prob):
    """prob as run_buckling.cpp reads it"""
    xy, conn = prob.mesh.xy.reshape(-1, 2), prob.mesh.conn.reshape(-1, 3)
    known, u, f = prob.u_known.reshape(-1, 2), prob.u_in.reshape(-1, 2), prob.f_in.reshape(-1, 2)
    h = lambda v: float(v).hex()
    lines = [f"{len(xy)} {len(conn)} {h(prob.youngs_modulus)} {h(prob.poisson_ratio)} {h(prob.part_thickness)}"]
    for i in range(len(xy)):
        lines.append(" ".join([h(xy[i, 0]), h(xy[i, 1]), str(int(known[i, 0])), str(int(known[i, 1])), h(u[i, 0]), h(u[i, 1]), h(f[i, 0]), h(f[i, 1])]))
    lines += [" ".join(str(int(n)) for n in tri) for tri in conn]
    path.write_text("\n".join(lines) + "\n")


def test_cpp_buckling_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_buckling"))


def test_the_tool_still_parses_without_a_gpu(exe, tensile_files):
    d, _ = tensile_files
    r = subprocess.run([exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run", "--buckling", "4", "--subspace", "12"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "dry-run:" in r.stdout, r.stderr
    for bad in (["--buckling", "-1"], ["--subspace", "8"]):
        r = subprocess.run([exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "--buckling" in r.stderr, bad


@pytest.mark.gpu
def test_cpp_buckling_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    prob = ref.cached("column8")[0]
    write_problem(tmp_path / "column8.txt", prob)
    binary = str(tmp_path / "run_buckling")
    compile_to(binary)
    r = subprocess.run([binary, str(tmp_path / "column8.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    info = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "info"]
    modes = [ln for ln in lines if ln[0] == "mode"]
    x = 1.0 / (1.0 + np.arange(2 * prob.mesh.num_nodes))
    with Context(device=0) as c:
        got = c.buckling(prob, modes=6, subspace=14, max_outer=60)
        y, val = c.apply_geometric(x), c.assemble_geometric()
    assert got["converged"] == 1 and got["positive"] == 6
    assert info == [[got[k] for k in INFO]]
    assert [float.fromhex(ln[1]) for ln in lines if ln[0] == "critical"] == [got["critical"]]
    assert len(modes) == 6
    for k, row in enumerate(modes):
        assert [float.fromhex(v) for v in row[2:4]] == [got["load_factor"][k], got["residual"][k]], k
        assert float.fromhex(row[5]) == sum_in_order(got["shapes"][k]), k
    op, = [ln for ln in lines if ln[0] == "operator"]
    assert float.fromhex(op[1]) == sum_in_order(y) and float.fromhex(op[3]) == sum_in_order(val)


@pytest.mark.gpu
def test_the_tool_writes_the_buckling_modes_and_leaves_the_other_files_as_they_are(exe, tensile_files, tmp_path):
    from magnetite_amd import Context
    from magnetite_amd.inputs import problem_from_input
    from magnetite_amd.msh import parse_mesh
    from magnetite_amd.post_processor import _fmt
    d, g = tensile_files
    args = [exe, str(d / "input.json"), str(d / "geom.msh")]
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    outs = {}
    for where, extra in ((plain, []), (flagged, ["--buckling", "2", "--subspace", "8"])):
        where.mkdir()
        r = subprocess.run(args + ["--nodes", str(where / "nodes.csv"), "--elements", str(where / "elements.csv")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[where] = r.stdout
    assert sorted(os.listdir(plain)) == ["elements.csv", "nodes.csv"]
    assert "info: buckling mode " not in outs[plain]
    assert sorted(os.listdir(flagged)) == ["buckling_modes.csv", "elements.csv", "nodes.csv"]
    for name in ("nodes.csv", "elements.csv"):
        assert (plain / name).read_bytes() == (flagged / name).read_bytes(), name
    prob = problem_from_input(parse_mesh(str(d / "geom.msh")), str(d / "input.json"))
    turned = np.ascontiguousarray(prob.mesh.conn[:, ::-1])  # (all clockwise after check_ccw: the tool turns every element)
    with Context(device=0) as c:
        c.upload(prob.xy_flat, turned, prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
        c.run()
        got = c.buckling(modes=2, subspace=8)
    N = prob.mesh.num_nodes
    text = (flagged / "buckling_modes.csv").read_text().splitlines()
    assert text[0] == "id,ux1,uy1,ux2,uy2" and len(text) == N + 1
    for i in (0, 1, N // 2, N - 1):  # the reference's float formatting, digit for digit
        want = [str(i)] + [_fmt(got["shapes"][k, 2 * i + a]) for k in range(2) for a in (0, 1)]
        assert text[1 + i].split(",") == want, i
    lines = [ln.split() for ln in outs[flagged].splitlines() if ln.startswith("info: buckling mode ")]
    assert len(lines) == 2
    for k, ln in enumerate(lines):
        assert ln[3] == str(k + 1) and ln[4:6] == ["load", "factor"] and ln[7] == "residual"
        assert float(ln[6]) == got["load_factor"][k] and float(ln[8]) == got["residual"][k]
