"""-m gpu: full-size solves against a DIRECT solve, the TRUE residual under the oracle's matrix, and EVERY entry.

tests/test_fullsize_parity_gpu.py pins the library to the oracle's CG trajectory at bench.py's stop (relative 1e-8, 6e-7
away from the discrete solution on hole1m), at 4096 sampled positions.  This file closes what that leaves open:

  test_solution_at_round_off   hole1m / frontal1m under the library's DEFAULT options (the reference's stop rule,
      absolute 1e-4) and under MAG_STOP_RNORM_SQ, on chip (cg_variant 2; frontal1m runs the overflow edge blocks) and
      streaming (1), against tests/golden/roundoff_*.npz (generator: tests/golden/make_roundoff_fixtures.py):
      - the DIRECT solution (SuperLU + refinement, residual 5e-15): sampled u and |u| within TOL_U + d, d the fixture's
        recorded oracle-to-direct distance of that rule (triangle inequality; 2e-12 and 9e-10 on hole1m, so 1e-8 in
        effect).  This assertion does not pass through any CG restatement;
      - the oracle's CG under the same rule: u within TOL_U, f and stress within TOL_DERIVED, as the full-size test;
      - the iteration count within twice the largest difference on record (profiles/roundoff_parity.json).
  test_every_entry   plate100k, hole1m, frontal1m, plate4m, multihole16m (and the cases above), default options and bench.py's
      relative 1e-8, with K = oracle.assemble_sparse (tests/fullsize_checks.py; its bite is proven on the CPU by
      tests/test_fullsize_checks_cpu.py): true residual |(f_in - K u)[free]| / |b|, all 2N entries of u and f, all E
      stresses.  Residual bars:
      - MAG_STOP_REL: 1.05 x tol.  The kernels stop on the true r.r they carry, and at this stop the oracle's recurred
        and true residuals still agree to 6e-8 of their value (hole1m: 10.3468724 against 10.3468717), so 5 % is
        margin for another summation order and anything beyond it is drift;
      - absolute rules: by their stop the recurred residual HAS drifted (oracle on hole1m: recurred 9.95e-5, true
        2.28e-4), and the kernels expand beta from the previous iterate's dots, so theirs may drift differently: 4 x
        the oracle's own true residual for that workload and rule (roundoff_*.npz; a live oracle.run for plate100k).
      plate4m has no oracle solve under the default rule to measure against (15 minutes and more): MAG_STOP_REL only.
      multihole16m (the only size beyond the Infinity Cache) likewise: its oracle solve is the OpenMP one of the
      sampled fixture.  The oracle assembles its K (224M non-zeros) in about a second on 16 cores and the checks peak
      near 10 GB of host memory, so it joins under MAG_STOP_REL.

Set MAG_ROUNDOFF_RECORD=<file> to have every figure written out as JSON (scripts/roundoff_parity.py does, and adds the
iteration counts of the sampled full-size cases); every figure is recorded before it is judged.
PARITY UNPINNED against reference outputs (none exist).
"""
import json
import os

import numpy as np
import pytest

import fullsize_checks as fc
from magnetite_amd import Context, _lib, meshgen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_U, TOL_DERIVED, REL_TOL = 1e-8, 1e-7, 1e-8
RULES = {"rnorm": {}, "rnorm_sq": dict(stop_mode=_lib.MAG_STOP_RNORM_SQ),
         "rel": dict(stop_mode=_lib.MAG_STOP_REL, tol=REL_TOL)}
# |gpu - oracle| iterations <= max(2, 2 x the largest difference observed for the workload): profiles/roundoff_parity.json,
# "largest_iteration_difference" (all variants and stop rules of this file and the sampled cases of
# tests/test_fullsize_parity_gpu.py)
LARGEST_ITERATION_DIFFERENCE = {"hole1m": 0, "frontal1m": 90}
RECORD = {}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


class Workload:
    def __init__(self, name):
        self.name, self.p = name, meshgen.baseline_problem(name)
        path = os.path.join(GOLDEN, f"roundoff_{name}.npz")
        self.fx = np.load(path, allow_pickle=False) if os.path.exists(path) else None
        self._system = self._oracle_residual = None
        self._solves = {}

    @property
    def system(self):
        if self._system is None:
            self._system = fc.System(self.p)
        return self._system

    def solve(self, variant, rule, assemble_csr=1):
        key = (variant, rule, assemble_csr)
        if key not in self._solves:
            with Context(device=0, cg_variant=variant, assemble_csr=assemble_csr, **RULES[rule]) as c:
                self._solves[key] = c.solve(self.p)
        return self._solves[key]

    def oracle_true_residual(self, rule):
        """|b - K_ff x| / |b| of the ORACLE's CG under an absolute rule: the fixture's, or a live run's (plate100k)."""
        if self.fx is not None:
            return float(self.fx[f"{rule}_true_rel_residual"])
        assert self.name == "plate100k" and rule == "rnorm"
        if self._oracle_residual is None:
            import oracle
            p = self.p
            ref = oracle.run(p.xy_flat, p.conn_flat, p.u_known, p.u_in, p.f_in, p.youngs_modulus, p.poisson_ratio,
                             p.part_thickness, path="sparse")
            self._oracle_residual = self.system.residual(ref["u"])
        return self._oracle_residual


WORKLOADS = {}


@pytest.fixture
def workload(request, built):
    """A BASELINE workload with its K and its solves, each made once and kept while this module runs (both tests of a
    case share one solve; about 15 GB of host memory by the end, the 16M-triangle system being most of it)."""
    if request.param not in WORKLOADS:
        WORKLOADS[request.param] = Workload(request.param)
    return WORKLOADS[request.param]


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    WORKLOADS.clear()
    if os.environ.get("MAG_ROUNDOFF_RECORD"):
        with open(os.environ["MAG_ROUNDOFF_RECORD"], "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


def note(name, variant, rule, assemble_csr=1, **figures):
    RECORD.setdefault(f"{name} cg_variant={variant} {rule}" + ("" if assemble_csr else " assemble_csr=0"), {}).update(figures)
    print(name, variant, rule, assemble_csr, figures, flush=True)


ROUNDOFF_CASES = [(n, v, r) for n in ("hole1m", "frontal1m") for v in (2, 1) for r in ("rnorm", "rnorm_sq")]


@pytest.mark.parametrize("workload,variant,rule", ROUNDOFF_CASES, indirect=["workload"])
def test_solution_at_round_off(workload, variant, rule):
    w, fx, p = workload, workload.fx, workload.p
    N, E = p.mesh.num_nodes, p.mesh.num_elements
    assert (N, E) == (int(fx["num_nodes"]), int(fx["num_elements"]))
    assert float(np.sum(p.xy_flat * np.arange(1, 2 * N + 1) % 7.0)) == float(fx["xy_checksum"])
    assert int(np.sum(p.conn_flat.astype(np.int64) * (np.arange(3 * E) % 11 + 1))) == int(fx["conn_checksum"])
    out = w.solve(variant, rule)
    iu, ie, known = fx["dof_idx"], fx["elem_idx"], p.u_known == 1
    d = float(fx[f"{rule}_rel_l2_to_direct"])
    u_norm = float(np.linalg.norm(out["u"]))
    fig = dict(gpu_iterations=int(out["iterations"]), oracle_iterations=int(fx[f"{rule}_iterations"]),
               oracle_to_direct=d, u_to_direct=rel(out["u"][iu], fx["direct_u_at"]),
               u_norm_to_direct=abs(u_norm - float(fx["direct_u_norm"])) / float(fx["direct_u_norm"]),
               u_to_oracle=rel(out["u"][iu], fx[f"{rule}_u_at"]),
               f_to_oracle=float(np.abs(out["f"][iu] - fx[f"{rule}_f_at"]).max() / float(fx[f"{rule}_f_known_norm"])),
               stress_to_oracle=rel(out["stress"][ie], fx[f"{rule}_stress_at"]), gpu_final_cost=float(out["final_cost"]))
    note(w.name, variant, rule, **fig)
    assert out["converged"] == 1 and out["cg_kernel"] == variant and out["termination"] == _lib.MAG_TERM_TARGET_COST
    # against the direct solve
    assert fig["u_to_direct"] <= TOL_U + d
    assert fig["u_norm_to_direct"] <= TOL_U + d
    # against the oracle's CG under the same rule
    assert fig["u_to_oracle"] <= TOL_U
    assert abs(u_norm - float(fx[f"{rule}_u_norm"])) <= TOL_U * float(fx[f"{rule}_u_norm"])
    assert np.abs(out["u"]).max() == pytest.approx(float(fx[f"{rule}_u_absmax"]), rel=1e-9)
    fk = float(fx[f"{rule}_f_known_norm"])
    assert fig["f_to_oracle"] <= TOL_DERIVED
    assert abs(np.linalg.norm(out["f"][known]) - fk) <= TOL_DERIVED * fk
    assert fig["stress_to_oracle"] <= TOL_DERIVED
    sn = float(fx[f"{rule}_stress_norm"])
    assert abs(np.linalg.norm(out["stress"]) - sn) <= TOL_DERIVED * sn
    slack = max(2, 2 * LARGEST_ITERATION_DIFFERENCE[w.name])
    assert abs(fig["gpu_iterations"] - fig["oracle_iterations"]) <= slack


# (workload, cg_variant, stop rule, assemble_csr)
EVERY_ENTRY_CASES = (
    [("plate100k", v, r, 1) for v in (2, 1, 0) for r in ("rnorm", "rel")] +
    [("hole1m", v, r, 1) for v in (2, 1) for r in ("rnorm", "rnorm_sq", "rel")] +
    [("hole1m", v, "rnorm", 0) for v in (2, 1)] +  # reactions from the matrix-free operator
    [("frontal1m", v, r, 1) for v in (2, 1) for r in ("rnorm", "rnorm_sq", "rel")] +
    [("plate4m", 1, "rel", 1), ("multihole16m", 1, "rel", 1)])


@pytest.mark.parametrize("workload,variant,rule,assemble_csr", EVERY_ENTRY_CASES, indirect=["workload"])
def test_every_entry(workload, variant, rule, assemble_csr):
    w, s = workload, workload.system
    out = w.solve(variant, rule, assemble_csr)
    u, f, stress = out["u"], out["f"], out["stress"]
    bar = 1.05 * REL_TOL if rule == "rel" else 4 * w.oracle_true_residual(rule)
    fig = dict(gpu_iterations=int(out["iterations"]), gpu_final_cost=float(out["final_cost"]), stress_excluded=0)
    if rule != "rel":
        fig["oracle_true_residual"] = w.oracle_true_residual(rule)
    try:
        s.check_all(u, f, stress, bar, matrix_free=not assemble_csr, figures=fig)
    finally:
        note(w.name, variant, rule, assemble_csr, **fig)
    assert out["converged"] == 1 and out["cg_kernel"] == variant and out["termination"] == _lib.MAG_TERM_TARGET_COST
