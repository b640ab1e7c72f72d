"""mag_run_newton on the 100k-triangle plate as a cantilever under a tip load (the right edge pulled down by TOTAL_LOAD, spread over
its nodes), 8 increments, newton_tol and cg_tol 1e-10: the wall time of a Newton iteration split into force / tangent / gather / CG
(the pass's own events, MAG_TUNE_NEWTON_TIMES), median of 7 runs per leg with the legs alternated in one session, for cg = 0 (the
fused block-row kernel, block-Jacobi) and cg = 4 (the CSR operator's phase), against the same iteration on the host: the numpy
twin of tests/newton_ref.py (tangent + force) and a sparse LU of K_T,FF per iteration, every iteration of one run a sample.  The
final displacement of every leg is compared with the twin's (relative L2).
    python scripts/newton_probe.py [--out profiles/newton.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
REPEATS, INCREMENTS, TOTAL_LOAD = 7, 8, 3e8
LEGS = (0, 4)


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def cantilever(n):
    from magnetite_amd import meshgen
    mesh = meshgen.plate(n)
    prob = meshgen.config_fixed_left_point_load(mesh, load=0.0)
    x = mesh.xy[:, 0]
    right = np.flatnonzero(x > x.max() - 1e-9)
    prob.f_in[:] = 0.0
    prob.f_in[2 * right + 1] = -TOTAL_LOAD / len(right)
    return prob, right


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton.json"))
    ap.add_argument("--grid", type=int, default=224)
    a = ap.parse_args()
    import explicit_tl_ref as tl
    import newton_ref as nr
    import scipy.sparse.linalg as spla
    from magnetite_amd import Context
    prob, right = cantilever(a.grid)
    args = nr.of_problem(prob)
    known = np.asarray(prob.u_known).reshape(-1) != 0
    free = np.flatnonzero(~known)

    # ---- the device
    times = tempfile.NamedTemporaryFile(suffix=".jsonl", delete=False)
    times.close()
    os.environ["MAG_TUNE_NEWTON_TIMES"] = times.name
    wall = {cg: [] for cg in LEGS}
    last = {}
    with Context(device=0) as c:
        c.upload_problem(prob)
        for cg in LEGS:  # (the first run of a leg builds its tables)
            c.newton(increments=INCREMENTS, cg=cg)
        open(times.name, "w").close()
        for _ in range(REPEATS):
            for cg in LEGS:
                t0 = time.perf_counter()
                out = c.newton(increments=INCREMENTS, cg=cg)
                wall[cg].append(1e3 * (time.perf_counter() - t0))
                last[cg] = out
    rows = [json.loads(ln) for ln in open(times.name)]
    os.unlink(times.name)
    legs = {}
    for k, cg in enumerate(LEGS):
        mine = rows[k::len(LEGS)]
        out = last[cg]
        its = int(out["newton_iterations_total"])
        legs[f"cg{cg}"] = {
            "cg_kernel": int(out["cg_kernel"]), "preconditioner": int(out["preconditioner"]), "converged": int(out["converged"]),
            "newton_iterations": [int(v) for v in out["newton_iterations"]], "cg_iterations_total": int(out["cg_iterations_total"]),
            "min_det_F": float(out["elem"][:, 6].min()), "tip_uy": float(out["u"][2 * right + 1].mean()),
            "ms_run_wall": summary(wall[cg]),
            "ms_per_newton_iteration": {ph: summary([r[ph + "_ms"] / its for r in mine]) for ph in ("force", "tangent", "gather", "cg")},
            "us_per_cg_iteration": summary([1e3 * r["cg_ms"] / r["cg_iterations"] for r in mine]),
        }

    # ---- the host: the twin's iteration, every iteration of one run a sample
    host = {"force": [], "tangent": [], "lu": []}
    u = np.zeros(known.size)
    f = np.where(known, 0.0, prob.f_in)
    iterations = []
    for k in range(1, INCREMENTS + 1):
        lam = k / INCREMENTS
        for it in range(25):
            t0 = time.perf_counter()
            fi = tl.tl_force(*args, u)[0]
            t1 = time.perf_counter()
            K = nr.tangent(*args, u)
            t2 = time.perf_counter()
            r = (lam * f - fi)[free]
            if it > 0 and np.linalg.norm(r) <= 1e-10 * max(np.linalg.norm(lam * f), np.linalg.norm(fi[known])):
                iterations.append(it)
                break
            u[free] += spla.splu(K[free][:, free].tocsc()).solve(r)
            t3 = time.perf_counter()
            host["force"].append(1e3 * (t1 - t0))
            host["tangent"].append(1e3 * (t2 - t1))
            host["lu"].append(1e3 * (t3 - t2))
    result = {
        "mesh": f"plate {a.grid} x {a.grid}", "nodes": int(prob.mesh.num_nodes), "elements": int(prob.mesh.num_elements), "increments": INCREMENTS,
        "total_load": TOTAL_LOAD, "newton_tol": 1e-10, "cg_tol": 1e-10, "device": legs,
        "host": {"newton_iterations": iterations, "ms_per_newton_iteration": {k: summary(v) for k, v in host.items()}},
        "rel_u_against_the_host": {f"cg{cg}": float(np.linalg.norm(last[cg]["u"] - u) / np.linalg.norm(u)) for cg in LEGS},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
