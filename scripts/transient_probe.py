"""mag_run_transient on the 100k-triangle plate under the cantilever load applied at t = 0: 256 steps at dt = T1 / 200 for
cg = 1, 2, 3, 4 (fused plain / Jacobi / block-Jacobi on A's block rows, the CSR operator's phase), cg_tol 1e-10, median of 7
with the legs alternated in one session, against the twin of tests/transient_ref.py on the host (one sparse LU factorisation of
A_FF and a solve per step).

Per leg: ms per step, CG iterations per step, and -- from a fit  wall = steps * c_step + iterations * c_iteration  over the runs
at cg_tol 1e-6, 1e-10 and 1e-12 (least squares, every repeat a point) -- us per CG iteration and ms per step outside the CG.
The yardstick for the per-iteration figure is profiles/field_cg.json (the same kernel under a graph: 6.3-7.2 us).  The final
displacement of every leg is compared with the twin's (relative L2).
    python scripts/transient_probe.py [--out profiles/transient.json]"""
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
REPEATS, FIT_REPEATS, STEPS, RHO = 7, 3, 256, 2700.0
LEGS = (1, 2, 3, 4)
TOLS = (1e-6, 1e-10, 1e-12)


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transient.json"))
    ap.add_argument("--mesh", default="plate100k")
    a = ap.parse_args()
    import modal_ref
    import transient_ref as ref
    from magnetite_amd import Context, meshgen
    prob = meshgen.baseline_problem(a.mesh)
    K, M, free = modal_ref.matrices(prob, RHO)
    lam, _ = modal_ref.eigenpairs(K, M, free, 2)
    T1 = 2.0 * np.pi / float(np.sqrt(lam[0]))
    dt = T1 / 200.0

    # ---- the host: one factorisation, a solve per step
    spent = {"factor": 0.0, "solves": 0.0}

    def timed_lu(A):
        t0 = time.perf_counter()
        solve = ref.lu_solver(A)
        spent["factor"] += time.perf_counter() - t0

        def run(b):
            t0 = time.perf_counter()
            x = solve(b)
            spent["solves"] += time.perf_counter() - t0
            return x
        return run

    t0 = time.perf_counter()
    twin = ref.newmark(K, M, free, prob.u_in, prob.f_in, STEPS, dt, solver=timed_lu)
    host_wall = time.perf_counter() - t0
    host = {"wall_ms_per_step": round(1e3 * host_wall / STEPS, 4), "factorisations_ms": round(1e3 * spent["factor"], 3),
            "solve_ms_per_step": round(1e3 * spent["solves"] / (STEPS + 1), 4)}
    print("host", json.dumps(host), flush=True)

    # ---- the device: the legs alternated
    wall = {(cg, tol): [] for cg in LEGS for tol in TOLS}
    its = {}
    err = {}
    with Context(device=0) as c:
        c.upload_problem(prob)
        for cg in LEGS:  # (order, pattern, K, the buffers)
            c.run_transient(4, dt, RHO, cg=cg)
        for tol in TOLS:
            for rep in range(REPEATS if tol == 1e-10 else FIT_REPEATS):
                for cg in LEGS:
                    t0 = time.perf_counter()
                    c.run_transient(STEPS, dt, RHO, cg=cg, cg_tol=tol)
                    wall[cg, tol].append(1e3 * (time.perf_counter() - t0))
                    info = c.transient_info()
                    assert its.setdefault((cg, tol), info["cg_iterations"]) == info["cg_iterations"]
                    if rep == 0 and tol == 1e-10:
                        u = c.download_transient()["u"]
                        err[cg] = float(np.linalg.norm(u - twin["u"][-1]) / np.linalg.norm(twin["u"][-1]))
    out = {"mesh": a.mesh, "nodes": prob.mesh.num_nodes, "elements": prob.mesh.num_elements, "steps": STEPS, "dt": dt, "T1": T1,
           "cg_tol": 1e-10, "repeats": REPEATS, "host_sparse_lu": host, "legs": {}}
    for cg in LEGS:
        # the a_0 solve counts among the iterations and not among the steps: one more unknown would not be resolved by three tolerances
        rows = np.array([[STEPS, its[cg, tol]] for tol in TOLS for _ in wall[cg, tol]], dtype=np.float64)
        y = np.array([w for tol in TOLS for w in wall[cg, tol]])
        (c_step, c_it), *_ = np.linalg.lstsq(rows, y, rcond=None)
        w = wall[cg, 1e-10]
        out["legs"][str(cg)] = {
            "cg_kernel": 3 if cg == 4 else 5, "preconditioner": 0 if cg == 4 else cg - 1,
            "ms_per_step": summary([x / STEPS for x in w]), "iterations_per_step": round(its[cg, 1e-10] / STEPS, 3),
            "iterations_by_tolerance": {str(tol): its[cg, tol] for tol in TOLS},
            "us_per_cg_iteration_fit": round(1e3 * float(c_it), 4), "ms_per_step_outside_the_cg_fit": round(float(c_step), 5),
            "final_u_against_the_twin": err[cg],
            "host_over_device": round(host["wall_ms_per_step"] / (statistics.median(w) / STEPS), 3)}
        print("cg", cg, json.dumps(out["legs"][str(cg)]), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
