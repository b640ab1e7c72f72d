"""include/magnetite_solver.hpp, solver::run_explicit and solver::explicit_dt, and tools/magnetite_gpu.cpp --explicit: both compile
against the C ABI on any box and -- on the GPU box -- return for plate16 exactly the bits the Python binding returns; the tool
prints the step, a line per recorded row and writes history.csv next to nodes.csv / elements.csv, which stay byte for byte what
they are without the flag.

The tool's mesh reader turns every small element clockwise (the reference's check_ccw compares the area with 1.0) and
mag_run_explicit refuses such a mesh: the tool turns the elements back by their true sign, and so does the Python leg here."""
import json
import os
import subprocess

import numpy as np
import pytest

import explicit_cases as cases
import modal_ref
from magnetite_amd import meshgen
from magnetite_amd.inputs import problem_from_input
from magnetite_amd.msh import parse_mesh, write_msh
from test_cpp_driver import exe  # noqa: F401 (fixture)
from test_design_cpp import write_problem
from test_variants_cpp import sum_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "run_explicit.cpp")
RHO = cases.RHO
INFO = ("steps", "fused", "step_launches", "record_every", "snapshots_kept", "resumed")
PLATE_JSON = {
    "metadata": {"part_thickness": 0.5, "material_elasticity": 69e9, "poisson_ratio": 0.33,
                 "characteristic_length_min": 0, "characteristic_length_max": 0.3},
    "boundary_conditions": {
        "restraint": {"region": {"x_target_min": -1, "x_target_max": 1e-9}, "targets": {"ux": 0, "uy": 0, "fx": None, "fy": None}},
        "load": {"region": {"x_target_min": 1 - 1e-9, "x_target_max": 2}, "targets": {"ux": 1e-3, "uy": None, "fx": None, "fy": 0}},
    },
}


def compile_to(path):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", path,
           "-L", os.path.join(ROOT, "magnetite_amd"), "-lmagnetite_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "magnetite_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


@pytest.fixture(scope="module")
def plate_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("plate16")
    write_msh(meshgen.plate(16), str(d / "geom.msh"))
    (d / "input.json").write_text(json.dumps(PLATE_JSON))
    return d


def test_cpp_explicit_compiles_and_links(built, tmp_path):
    compile_to(str(tmp_path / "run_explicit"))


def test_the_tool_parses_the_flags_without_a_gpu(exe, plate_files):
    d = plate_files
    base = [exe, str(d / "input.json"), str(d / "geom.msh"), "--dry-run"]
    r = subprocess.run(base + ["--explicit", "64", "--density", "2700", "--dt-scale", "0.5", "--rayleigh", "0.5,1e-7", "--probe", "3", "--probe", "8",
                               "--record-every", "4"], capture_output=True, text=True)
    assert r.returncode == 0 and "dry-run: nodes 289 elements 512" in r.stdout, r.stdout + r.stderr
    assert "dry-run: explicit steps 64 dt 0 dt_scale 0.5 density 2700 rayleigh 0.5,0.0000001 probes 2 record_every 4" in r.stdout, r.stdout
    r = subprocess.run(base + ["--explicit", "64", "--density", "2700", "--dt", "2e-6"], capture_output=True, text=True)
    assert r.returncode == 0 and "dry-run: explicit steps 64 dt 0.000002 dt_scale 0 density 2700 rayleigh 0,0 probes 0 record_every 1" in r.stdout
    for wrong in (["--explicit", "64"], ["--explicit", "0", "--density", "2700"], ["--explicit", "4", "--density", "2700", "--dt", "1e-6", "--dt-scale", "0.5"],
                  ["--explicit", "4", "--density", "2700", "--record-every", "0"], ["--explicit", "4", "--density", "2700", "--rayleigh", "-1,0"]):
        r = subprocess.run(base + wrong, capture_output=True, text=True)
        assert r.returncode == 1 and "--explicit" in r.stderr and "--density" in r.stderr, (wrong, r.stderr)
    r = subprocess.run(base + ["--explicit", "4", "--density", "2700", "--transient", "4", "--dt", "1e-6"], capture_output=True, text=True)
    assert r.returncode == 1 and "one of them at a time" in r.stderr
    for alone in (["--dt-scale", "0.5"], ["--record-every", "2"]):
        r = subprocess.run(base + alone, capture_output=True, text=True)
        assert r.returncode == 1 and "--explicit" in r.stderr, (alone, r.stderr)


@pytest.mark.gpu
def test_cpp_explicit_equals_the_python_binding_bitwise(built, tmp_path):
    from magnetite_amd import Context
    prob, K, M, m, free, w1, T1 = cases.setup("plate16", "pull")
    alpha, eta = cases.rayleigh("damped", w1)
    N = prob.mesh.num_nodes
    write_problem(tmp_path / "plate16.txt", prob)
    binary = str(tmp_path / "run_explicit")
    compile_to(binary)
    r = subprocess.run([binary, str(tmp_path / "plate16.txt"), float(alpha).hex(), float(eta).hex()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    with Context(device=0) as c:
        c.upload_problem(prob)
        bound = c.explicit_dt(RHO, eta)
        got = c.explicit(steps=40, density=RHO, rayleigh=(alpha, eta), energies=True, record_every=4, snapshot_every=8, probes=[3, N, 2 * N - 1])
    assert got["fused"] == 1 and np.any(got["v"] != 0)
    assert [[float.fromhex(v) for v in ln[1:]] for ln in lines if ln[0] == "bound"] == [list(bound.values())]
    assert [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "info"] == [[got[k] for k in INFO]]
    assert [[float.fromhex(v) for v in ln[1:]] for ln in lines if ln[0] == "time"] == [[got["t_start"], got["t_end"], got["dt"], got["dt_bound"]]]
    sums = {ln[1]: float.fromhex(ln[2]) for ln in lines if ln[0] == "sum"}
    assert set(sums) == {"u", "v", "a", "f", "snapshots", "energies", "time"}
    for k, v in sums.items():
        assert v == sum_in_order(got[k].reshape(-1)), k
    rows = [ln for ln in lines if ln[0] == "row"]
    assert len(rows) == 11
    for n, row in enumerate(rows):
        want = [got[k][n, p] for p in range(3) for k in ("probe_u", "probe_v", "probe_a")]
        assert [float.fromhex(v) for v in row[2:]] == want, n


@pytest.mark.gpu
def test_the_tool_writes_the_history_and_leaves_the_other_files_as_they_are(exe, plate_files, tmp_path):
    from magnetite_amd import Context
    from magnetite_amd.post_processor import _fmt
    d = plate_files
    args = [exe, str(d / "input.json"), str(d / "geom.msh")]
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    outs = {}
    prob = problem_from_input(parse_mesh(str(d / "geom.msh")), str(d / "input.json"))
    N = prob.mesh.num_nodes
    probes = [3, N, 2 * N - 1]
    extra = ["--explicit", "40", "--density", "2700", "--dt-scale", "0.5", "--rayleigh", "3,1e-8", "--record-every", "4"] + \
        [w for p in probes for w in ("--probe", str(p))]
    for where, flags in ((plain, []), (flagged, extra)):
        where.mkdir()
        r = subprocess.run(args + ["--nodes", str(where / "nodes.csv"), "--elements", str(where / "elements.csv")] + flags,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[where] = r.stdout
    assert sorted(os.listdir(plain)) == ["elements.csv", "nodes.csv"]
    assert "info: step " not in outs[plain] and "info: explicit" not in outs[plain]
    assert sorted(os.listdir(flagged)) == ["elements.csv", "history.csv", "nodes.csv"]
    for name in ("nodes.csv", "elements.csv"):
        assert (plain / name).read_bytes() == (flagged / name).read_bytes(), name
    conn = np.array(prob.mesh.conn)
    clockwise = modal_ref.signed_areas(prob.mesh.xy, conn) < 0.0  # (the tool turns these back)
    conn[clockwise] = conn[clockwise][:, ::-1]
    with Context(device=0) as c:
        c.upload(prob.xy_flat, np.ascontiguousarray(conn), prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio,
                 prob.part_thickness)
        got = c.explicit(steps=40, density=RHO, dt_scale=0.5, rayleigh=(3.0, 1e-8), record_every=4, probes=probes)
    assert f"info: explicit dt {_fmt(got['dt'])} (bound {_fmt(got['dt_bound'])})" in outs[flagged].splitlines()
    text = (flagged / "history.csv").read_text().splitlines()
    assert text[0] == "step,t," + ",".join(f"u{p},v{p},a{p}" for p in probes) and len(text) == 12
    for n in range(11):  # the reference's float formatting, digit for digit
        want = [str(4 * n), _fmt(got["time"][n])] + [_fmt(got[k][n, p]) for p in range(3) for k in ("probe_u", "probe_v", "probe_a")]
        assert text[1 + n].split(",") == want, n
    lines = [ln.split() for ln in outs[flagged].splitlines() if ln.startswith("info: step ")]
    assert len(lines) == 11
    for n, ln in enumerate(lines):
        assert ln[2] == str(4 * n) and ln[3] == "t" and float(ln[4]) == got["time"][n]
