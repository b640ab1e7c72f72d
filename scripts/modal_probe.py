"""Context.modal() against what a user could do before it existed: the same subspace iteration driven from Python on the same
library -- solve_cases-style load sets (0, Y_j) for the q inner solves under MAG_STOP_REL, a scipy-built mass matrix, the
Rayleigh-Ritz step in numpy, the same start vectors and tolerances (tests/modal_ref.py, subspace_iteration).

p = 6 (q = 12) on the 3k-node holes mesh and on the 100k-triangle plate, density 2700.  After a warm-up of each leg, REPEATS
repeats, the two legs alternating: median and spread (max - min) of the host's wall time (each call ends in a device
synchronise).  Both legs' outer steps, the CG iterations of their last outer step, and the largest relative difference of
their eigenvalues are recorded next to the times.
    python scripts/modal_probe.py [--out profiles/modal.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
REPEATS = 7
RHO, MODES, SUBSPACE, TOL, CG_TOL = 2700.0, 6, 12, 1e-10, 1e-10


def med(v):
    return {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "repeats": len(v)}


def from_python(ctx, prob, M, free):
    """the baseline leg: dict(lam, outer, cg_iterations_last_step)"""
    import modal_ref as ref
    last = {}

    def solve(Y):
        ctx.set_load_cases(np.zeros_like(Y), Y)
        ctx.run_cases()
        last["iterations"] = sum(ctx.case_stats(j)["iterations"] for j in range(len(Y)))
        return np.stack([ctx.download_case(j)[0] for j in range(len(Y))])

    out = ref.subspace_iteration(None, M, free, ref.start_vectors(prob.mesh.xy, prob.u_known, SUBSPACE), MODES,
                                 tol=TOL, max_outer=50, solve=solve)
    out["cg_iterations_last_step"] = last["iterations"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modal.json"))
    a = ap.parse_args()
    import modal_ref as ref
    from magnetite_amd import Context, meshgen
    from magnetite_amd._lib import MAG_STOP_REL
    rows = []
    for name, make in (("holes3k", lambda: meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3))),
                       ("plate100k", lambda: meshgen.baseline_problem("plate100k"))):
        prob = make()
        M = ref.mass(prob.mesh.xy, prob.mesh.conn, RHO, prob.part_thickness)
        free = np.flatnonzero(np.asarray(prob.u_known) == 0)
        legs = {"modal": [], "from_python": []}
        with Context(device=0) as c, Context(device=0, stop_mode=MAG_STOP_REL, tol=CG_TOL) as base:
            base.upload_problem(prob)
            got = c.modal(prob, modes=MODES, density=RHO, subspace=SUBSPACE, tol=TOL, cg_tol=CG_TOL)  # warm-up
            want = from_python(base, prob, M, free)
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                got = c.modal(modes=MODES, density=RHO, subspace=SUBSPACE, tol=TOL, cg_tol=CG_TOL)
                t1 = time.perf_counter()
                want = from_python(base, prob, M, free)
                t2 = time.perf_counter()
                legs["modal"].append((t1 - t0) * 1e3)
                legs["from_python"].append((t2 - t1) * 1e3)
            last = sum(c.modal_stats(j)["iterations"] for j in range(SUBSPACE))
        row = {"mesh": name, "nodes": prob.mesh.num_nodes, "elements": prob.mesh.num_elements, "modes": MODES, "subspace": SUBSPACE}
        row.update({k: med(v) for k, v in legs.items()})
        row["speedup"] = round(statistics.median(legs["from_python"]) / statistics.median(legs["modal"]), 2)
        row["modal_outer"], row["modal_converged"] = got["outer"], got["converged"]
        row["modal_vectors_per_launch"], row["modal_launches"] = got["vectors_per_launch"], got["launches"]
        row["modal_cg_iterations_last_step"] = int(last)
        row["from_python_outer"], row["from_python_converged"] = want["outer"], want["converged"]
        row["from_python_cg_iterations_last_step"] = int(want["cg_iterations_last_step"])
        row["frequency_hz"] = [float(v) for v in got["frequency"]]
        row["residual_max"] = float(got["residual"].max())
        row["rel_lambda_between_legs"] = float(np.max(np.abs(got["lambda"] - want["lam"]) / want["lam"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"repeats": REPEATS, "density": RHO, "tol": TOL, "cg_tol": CG_TOL, "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
