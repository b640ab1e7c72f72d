"""The neo-Hooke material of the total-Lagrangian passes (mag_set_material_law) on the 100k-triangle plate: what the local solve of
the plane-stress condition, three times per (node, triangle), costs the fused explicit step, and what it costs the force and the
tangent launch of a Newton iteration.  Medians of 7, the legs alternated in one session.

The fused explicit step (4096 steps without records at 0.9 dt_bound, scripts/newton_probe.py's cantilever load applied at t = 0):
  (a) under MAG_LAW_NEO_HOOKE, (b) under MAG_LAW_SVK in this build -- alternated in one context;
  (c) under St. Venant-Kirchhoff in a child process of this build's library and (d) of the PARENT commit's (--parent-lib, loaded
      through MAG_LIB_PATH; it has no mag_set_material_law and is never asked for it).  (c) and (d) run alike, one after the other:
      they should agree within their spread, since nothing the St. Venant-Kirchhoff step runs has changed.  Without --parent-lib this
      build's library runs leg (d) too and the file says so.
One Newton iteration (mag_run_newton, 4 increments of the cantilever load, the pass's own events: MAG_TUNE_NEWTON_TIMES): the force
and the tangent launches per iteration under both laws, alternated.
    python scripts/hyper_probe.py [--parent-lib PATH] [--out profiles/hyper.json]"""
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
REPEATS, STEPS, RHO, INCREMENTS = 7, 4096, 2700.0, 4
LAWS = ("neo_hooke", "svk")


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def svk_leg(a):
    """child process: the total-Lagrangian step of whatever library MAG_LIB_PATH names, as it comes (St. Venant-Kirchhoff); one JSON line"""
    from magnetite_amd import Context
    from newton_probe import cantilever
    prob = cantilever(a.grid)[0]
    wall = []
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.run_explicit(8, dt=a.dt, density=RHO, kinematics="tl")
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            c.run_explicit(STEPS, dt=a.dt, density=RHO, kinematics="tl")
            wall.append(1e3 * (time.perf_counter() - t0))
        u = c.download_transient()["u"]
    print(json.dumps({"wall_ms": wall, "u_norm": float(np.linalg.norm(u))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyper.json"))
    ap.add_argument("--grid", type=int, default=224)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--svk-leg", action="store_true")
    ap.add_argument("--dt", type=float, default=0.0)
    a = ap.parse_args()
    if a.svk_leg:
        return svk_leg(a)
    from magnetite_amd import Context
    from newton_probe import cantilever
    prob = cantilever(a.grid)[0]
    N, E = prob.mesh.num_nodes, prob.mesh.num_elements

    times = tempfile.NamedTemporaryFile(suffix=".jsonl", delete=False)
    times.close()
    wall = {law: [] for law in LAWS}
    info, u, newton = {}, {}, {}
    with Context(device=0) as c:
        c.upload_problem(prob)
        dt = 0.9 * c.explicit_dt(RHO)["dt_bound"]
        for law in LAWS:  # (order, pattern, K, the buffers)
            c.set_material_law(law)
            c.run_explicit(8, dt=dt, density=RHO, kinematics="tl")
        for _ in range(REPEATS):
            for law in LAWS:
                c.set_material_law(law)
                t0 = time.perf_counter()
                c.run_explicit(STEPS, dt=dt, density=RHO, kinematics="tl")
                wall[law].append(1e3 * (time.perf_counter() - t0))
                info[law] = c.transient_info()
                u[law] = c.download_transient()["u"]
        # ---- a Newton iteration's force and tangent launches
        for law in LAWS:
            c.set_material_law(law)
            c.newton(increments=INCREMENTS)
        os.environ["MAG_TUNE_NEWTON_TIMES"] = times.name
        for _ in range(REPEATS):
            for law in LAWS:
                c.set_material_law(law)
                newton[law] = c.newton(increments=INCREMENTS)
        del os.environ["MAG_TUNE_NEWTON_TIMES"]
    for law in LAWS:  # a step without records is one launch (words 2 and 3), of the total-Lagrangian kernel
        assert (info[law]["preconditioner"], info[law]["cg_iterations"], info[law]["cg_kernel"]) == (1, STEPS + 1, 7), info[law]
    rows = [json.loads(ln) for ln in open(times.name)]
    os.unlink(times.name)

    children = {}
    for name, lib in (("this_build", None), ("parent", a.parent_lib)):
        env = dict(os.environ)
        if lib:
            env["MAG_LIB_PATH"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--svk-leg", "--grid", str(a.grid), "--dt", repr(dt)], env=env, capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        children[name] = json.loads(r.stdout.strip().splitlines()[-1])

    us = {law: 1e3 * statistics.median(wall[law]) / STEPS for law in LAWS}
    child_us = {k: 1e3 * statistics.median(v["wall_ms"]) / STEPS for k, v in children.items()}
    out = {"mesh": f"plate {a.grid} x {a.grid}", "nodes": N, "elements": E, "dt": dt, "steps": STEPS, "repeats": REPEATS,
           "explicit_step": {law: {"wall_ms": summary(wall[law]), "us_per_step": round(us[law], 4)} for law in LAWS},
           "neo_hooke_over_svk": round(us["neo_hooke"] / us["svk"], 3),
           "final_u_neo_hooke_against_svk": float(np.linalg.norm(u["neo_hooke"] - u["svk"]) / np.linalg.norm(u["svk"])),
           "svk_step_in_a_child_process": {
               "this_build": {"wall_ms": summary(children["this_build"]["wall_ms"]), "us_per_step": round(child_us["this_build"], 4)},
               "parent": {"library": "parent commit (MAG_LIB_PATH)" if a.parent_lib else "this build (no --parent-lib given)",
                          "wall_ms": summary(children["parent"]["wall_ms"]), "us_per_step": round(child_us["parent"], 4)},
               "this_build_over_parent": round(child_us["this_build"] / child_us["parent"], 3),
               "final_u_norm_equal": children["this_build"]["u_norm"] == children["parent"]["u_norm"]},
           "newton_iteration": {}}
    for k, law in enumerate(LAWS):
        mine = rows[k::len(LAWS)]
        its = int(newton[law]["newton_iterations_total"])
        out["newton_iteration"][law] = {"newton_iterations": [int(v) for v in newton[law]["newton_iterations"]], "converged": int(newton[law]["converged"]),
                                        "ms_per_iteration": {ph: summary([r[ph + "_ms"] / its for r in mine]) for ph in ("force", "tangent")}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
