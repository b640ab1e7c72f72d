"""mag_run_transient_tl on the 100k-triangle plate as scripts/newton_probe.py's cantilever under a step load (the right edge pulled
down by TOTAL_LOAD at t = 0), 64 steps at T1 / 50 with the lumped mass, newton_tol 1e-10 and cg_tol 1e-10, against the two things a
user has without the pass, both on the PARENT commit's library (--parent-lib, loaded by a child process through MAG_LIB_PATH):
  explicit   mag_run_explicit(kinematics = tl) over the same physical time at the largest dt <= 0.9 dt_bound that divides T1 / 50
             (what follows a large rotation today);
  linear     mag_run_transient at the same dt (the linear cost of one solve a step; not the same physics).
Every leg is a child process per round (one library per process), a short run first (tables, allocations), then the timed run;
the legs alternate over REPEATS rounds in one session, medians are reported.  The implicit leg also reads the pass's own phase
times (MAG_TUNE_TRANSIENT_TL_TIMES; `cg` is the CG alone, `state` the moves into and out of the solver's numbering + state + force +
residual): the CG's share of a step, microseconds per CG iteration, and what a Newton iteration costs outside the CG.  The tip's
history of the implicit leg is compared with the explicit leg's at the same times.
    python scripts/transient_tl_probe.py --parent-lib DIR/libmagnetite_hip.so [--out profiles/transient_tl.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS, STEPS, DIV, TOTAL_LOAD, RHO = 7, 64, 50, 3e8, 2700.0
LEGS = ("implicit", "explicit", "linear")


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


def child(leg, grid, dt, per_step):
    """one leg in this process's library: a short run, then the timed one; one JSON line"""
    from magnetite_amd import Context
    prob, right = cantilever(grid)
    tip = [int(2 * right[len(right) // 2] + 1)]
    with Context(device=0) as c:
        c.upload_problem(prob)
        if leg == "implicit":
            kw = dict(dt=dt, density=RHO, lumped=True, kinematics="tl", newton_tol=1e-10, cg_tol=1e-10, probes=tip)
            c.transient(steps=2, **kw)
            times = tempfile.NamedTemporaryFile(suffix=".jsonl", delete=False)
            times.close()
            os.environ["MAG_TUNE_TRANSIENT_TL_TIMES"] = times.name
            t0 = time.perf_counter()
            out = c.transient(steps=STEPS, **kw)
            ms = 1e3 * (time.perf_counter() - t0)
            phases = json.loads(open(times.name).read().splitlines()[-1])
            os.unlink(times.name)
            extra = dict(phases=phases, newton_iterations=[int(v) for v in out["newton_iterations"]], converged=int(out["converged"]),
                         cg_iterations_total=int(out["cg_iterations_total"]), min_det_F=float(out["elements"][:, 6].min()),
                         cg_kernel=int(out["cg_kernel"]), preconditioner=int(out["preconditioner"]))
        elif leg == "explicit":
            kw = dict(dt=dt / per_step, density=RHO, kinematics="tl", probes=tip, record_every=per_step)
            c.explicit(steps=2 * per_step, **kw)
            t0 = time.perf_counter()
            out = c.explicit(steps=STEPS * per_step, **kw)
            ms = 1e3 * (time.perf_counter() - t0)
            extra = dict(dt=float(out["dt"]), dt_bound=float(out["dt_bound"]), steps=int(out["steps"]), fused=int(out["fused"]),
                         inverted=bool(out["inverted"]))
        else:
            kw = dict(dt=dt, density=RHO, lumped=True, cg_tol=1e-10, probes=tip)
            c.transient(steps=2, **kw)
            t0 = time.perf_counter()
            out = c.transient(steps=STEPS, **kw)
            ms = 1e3 * (time.perf_counter() - t0)
            extra = dict(cg_iterations=int(out["cg_iterations"]), converged=int(out["converged"]))
    print(json.dumps(dict(leg=leg, ms=ms, tip=[float(v) for v in out["probe_u"][:, 0]], **extra)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transient_tl.json"))
    ap.add_argument("--grid", type=int, default=224)
    ap.add_argument("--parent-lib", required=True, help="libmagnetite_hip.so of the parent commit's build")
    ap.add_argument("--child", nargs=3, metavar=("LEG", "DT", "PER_STEP"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.grid, float.fromhex(a.child[1]), int(a.child[2]))
    from magnetite_amd import Context
    prob, _ = cantilever(a.grid)
    with Context(device=0) as c:  # the period and the explicit bound, on the device
        c.upload_problem(prob)
        T1 = 1.0 / float(c.modal(modes=1, density=RHO, lumped=True)["frequency"][0])
        bound = c.explicit_dt(RHO)["dt_bound"]
    dt = T1 / DIV
    per_step = int(np.ceil(dt / (0.9 * bound)))
    runs = {leg: [] for leg in LEGS}
    for _ in range(REPEATS):
        for leg in LEGS:
            env = dict(os.environ)
            if leg != "implicit":
                env["MAG_LIB_PATH"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--grid", str(a.grid), "--parent-lib", a.parent_lib, "--child", leg,
                                float(dt).hex(), str(per_step)], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:  # (a leg that failed ends the session: nothing more is started)
                sys.exit(f"leg {leg} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[leg].append(json.loads(r.stdout.strip().splitlines()[-1]))
    imp, exp, lin = (runs[leg] for leg in LEGS)
    its = sum(imp[-1]["newton_iterations"])
    ph = [r["phases"] for r in imp]
    outside = [(p["tangent_ms"] + p["gather_ms"] + p["state_ms"]) / p["newton_iterations"] for p in ph]
    rows = min(len(imp[-1]["tip"]), len(exp[-1]["tip"]))  # (an implicit run that ended early has fewer)
    tip_i, tip_e = np.array(imp[-1]["tip"][:rows]), np.array(exp[-1]["tip"][:rows])
    result = {
        "mesh": f"plate {a.grid} x {a.grid}", "nodes": int(prob.mesh.num_nodes), "elements": int(prob.mesh.num_elements), "steps": STEPS,
        "T1": T1, "dt": dt, "dt_over_explicit_bound": dt / bound, "total_load": TOTAL_LOAD, "mass": "lumped", "newton_tol": 1e-10, "cg_tol": 1e-10,
        "implicit": {
            "library": "this build", "cg_kernel": imp[-1]["cg_kernel"], "preconditioner": imp[-1]["preconditioner"], "converged": imp[-1]["converged"],
            "newton_iterations_per_step": its / STEPS, "newton_iterations": imp[-1]["newton_iterations"],
            "cg_iterations_total": imp[-1]["cg_iterations_total"], "min_det_F": imp[-1]["min_det_F"],
            "ms_run": summary([r["ms"] for r in imp]), "ms_per_step": summary([r["ms"] / STEPS for r in imp]),
            "cg_share_of_the_iterations": summary([p["cg_ms"] / (p["tangent_ms"] + p["gather_ms"] + p["cg_ms"] + p["state_ms"]) for p in ph]),
            "cg_share_of_the_run": summary([p["cg_ms"] / r["ms"] for p, r in zip(ph, imp)]),
            "us_per_cg_iteration": summary([1e3 * p["cg_ms"] / p["cg_iterations"] for p in ph]),
            "ms_per_newton_iteration_outside_the_cg": summary(outside),
            "ms_per_newton_iteration": {k: summary([p[k + "_ms"] / p["newton_iterations"] for p in ph]) for k in ("tangent", "gather", "cg", "state")},
        },
        "explicit_tl_on_the_parent": {
            "library": "the parent commit's build", "dt": exp[-1]["dt"], "dt_bound": exp[-1]["dt_bound"], "steps": exp[-1]["steps"],
            "steps_per_implicit_step": per_step, "fused": exp[-1]["fused"], "inverted": exp[-1]["inverted"],
            "ms_run": summary([r["ms"] for r in exp]), "ms_per_implicit_step": summary([r["ms"] / STEPS for r in exp]),
        },
        "linear_on_the_parent": {
            "library": "the parent commit's build", "cg_iterations": lin[-1]["cg_iterations"], "converged": lin[-1]["converged"],
            "ms_run": summary([r["ms"] for r in lin]), "ms_per_step": summary([r["ms"] / STEPS for r in lin]),
        },
        "implicit_over_explicit_run_time": statistics.median([r["ms"] for r in imp]) / statistics.median([r["ms"] for r in exp]),
        "implicit_over_linear_run_time": statistics.median([r["ms"] for r in imp]) / statistics.median([r["ms"] for r in lin]),
        "tip_uy": {"implicit_last": float(tip_i[-1]), "explicit_last": float(tip_e[-1]),
                   "history_difference_rel_l2": float(np.linalg.norm(tip_i - tip_e) / np.linalg.norm(tip_e)),
                   "largest_deflection_over_length": float(np.abs(tip_e).max() / np.ptp(prob.mesh.xy[:, 0]))},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
