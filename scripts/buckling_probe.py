"""Context.buckling() against what a user could do before it existed: the same subspace iteration driven from Python on the same
library -- solve_cases-style load sets (0, Y_j) for the q inner solves under MAG_STOP_REL, a scipy-built K_G of the downloaded
u0, the Ritz step in numpy, the same start vectors and tolerances (tests/buckling_ref.py, subspace_iteration).

The part: the 100k-triangle plate as a column -- fixed on the left, the right edge under a uniform compression of P in all.
p = 1 (q = 12): the critical factor (the square plate's next factors lie within 5 % of each other, and four of them do not settle
within the cap of 50 outer steps with 12 vectors; the first takes 18).  After a warm-up of each leg, REPEATS repeats, the two legs
alternating: median and spread (max - min) of the host's wall time (each call ends in a device synchronise; the prestress run is
outside both legs, the baseline's K_G is built once, outside its leg too).  Both legs' outer steps, the CG iterations of their last outer step, and the largest relative
difference of their factors are recorded next to the times.
    python scripts/buckling_probe.py [--out profiles/buckling.json]"""
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
MODES, SUBSPACE, TOL, CG_TOL, LOAD = 1, 12, 1e-10, 1e-10, 1e6


def med(v):
    return {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "repeats": len(v)}


def column_of_the_plate():
    """the mesh of the 100k-triangle baseline plate, fixed on the left, its right edge compressed by LOAD in all (weights 1, and 1/2 at
    the two corners)"""
    from magnetite_amd import meshgen
    prob = meshgen.config_fixed_left_point_load(meshgen.baseline_problem("plate100k").mesh)
    x, y = prob.mesh.xy[:, 0], prob.mesh.xy[:, 1]
    right = np.flatnonzero(x == x.max())
    w = np.ones(len(right))
    w[(y[right] == y[right].min()) | (y[right] == y[right].max())] = 0.5
    f = np.zeros_like(prob.f_in)
    f[2 * right] = -LOAD * w / w.sum()
    prob.f_in = f
    return prob


def from_python(ctx, prob, KG, free):
    """the baseline leg: dict(lam, outer, converged, cg_iterations_last_step)"""
    import buckling_ref as ref
    import modal_ref
    last = {}

    def solve(Y):
        ctx.set_load_cases(np.zeros_like(Y), Y)
        ctx.run_cases()
        last["iterations"] = sum(ctx.case_stats(j)["iterations"] for j in range(len(Y)))
        return np.stack([ctx.download_case(j)[0] for j in range(len(Y))])

    out = ref.subspace_iteration(None, KG, free, modal_ref.start_vectors(prob.mesh.xy, prob.u_known, SUBSPACE), MODES, tol=TOL, max_outer=50,
                                 solve=solve)
    out["cg_iterations_last_step"] = last["iterations"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "buckling.json"))
    ap.add_argument("--repeats", type=int, default=REPEATS)
    a = ap.parse_args()
    import buckling_ref as ref
    from magnetite_amd import Context
    from magnetite_amd._lib import MAG_STOP_REL
    prob = column_of_the_plate()
    free = np.flatnonzero(np.asarray(prob.u_known) == 0)
    legs = {"buckling": [], "from_python": []}
    with Context(device=0, stop_mode=MAG_STOP_REL, tol=1e-12) as c, Context(device=0, stop_mode=MAG_STOP_REL, tol=CG_TOL) as base:
        u0 = c.solve(prob)["u"]
        KG = ref.geometric_of(prob, u0)
        base.upload_problem(prob)
        got = c.buckling(modes=MODES, subspace=SUBSPACE, tol=TOL, cg_tol=CG_TOL)  # warm-up
        want = from_python(base, prob, KG, free)
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            got = c.buckling(modes=MODES, subspace=SUBSPACE, tol=TOL, cg_tol=CG_TOL)
            t1 = time.perf_counter()
            want = from_python(base, prob, KG, free)
            t2 = time.perf_counter()
            legs["buckling"].append((t1 - t0) * 1e3)
            legs["from_python"].append((t2 - t1) * 1e3)
        last = sum(c.buckling_stats(j)["iterations"] for j in range(SUBSPACE))
    row = {"mesh": "plate100k as a column", "nodes": prob.mesh.num_nodes, "elements": prob.mesh.num_elements, "modes": MODES, "subspace": SUBSPACE}
    row.update({k: med(v) for k, v in legs.items()})
    row["speedup"] = round(statistics.median(legs["from_python"]) / statistics.median(legs["buckling"]), 2)
    row["buckling_outer"], row["buckling_converged"] = got["outer"], got["converged"]
    row["buckling_vectors_per_launch"], row["buckling_launches"] = got["vectors_per_launch"], got["launches"]
    row["buckling_cg_iterations_last_step"] = int(last)
    row["from_python_outer"], row["from_python_converged"] = want["outer"], want["converged"]
    row["from_python_cg_iterations_last_step"] = int(want["cg_iterations_last_step"])
    row["load_factor"] = [float(v) for v in got["load_factor"]]
    row["residual_max"] = float(got["residual"].max())
    row["rel_factor_between_legs"] = float(np.max(np.abs(got["load_factor"] - want["lam"]) / np.abs(want["lam"])))
    print(json.dumps(row), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"repeats": a.repeats, "load": LOAD, "tol": TOL, "cg_tol": CG_TOL, "rows": [row]}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
