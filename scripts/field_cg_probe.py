"""mag_options.field_cg against the CSR operator's phase, on the 100k-triangle plate under the cantilever load: MAG_STOP_REL
1e-8, volume fraction 0.5, 20 iterations of the design loop (run + run_sensitivities + design_step) for field_cg 0, 1, 2, 3.

Per design iteration: CG iterations, ms_cg, us per CG iteration, ms_assemble, ms_csr_symbolic, the host's wall time of the whole
iteration.  Then, on the design the 20th iteration solved (its scale handed to a fresh context with set_element_scale), REPEATS
times run + run_sensitivities: median, min and max of the wall time, of ms_cg and of us per CG iteration.  The one-off build of
the block-row table is the first run's ms_csr_symbolic over leg 0's; the per-assembly gather and inverse blocks are ms_assemble
over leg 0's (both are inside those phases' event pairs, mag_run has no timer of their own).

The yardstick is the parent commit's library (--parent-lib, loaded by a child process through MAG_LIB_PATH) running this script's
leg 0 with no option set.  The new build's leg 0 must reproduce its iteration counts exactly -- otherwise the comparison is not
like for like and the probe fails.  Requirements (recorded as booleans, the numbers next to them): us per CG iteration of
field_cg 1 below the parent's by more than the parent's own min-max spread; the best leg's whole iteration below the parent's by
more than its spread.
    python scripts/field_cg_probe.py --parent-lib PATH [--out profiles/field_cg.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
REPEATS = 7
ITERS = 20


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def leg(kind, tol):
    """one leg in this process, with the library this process loaded; kind None: no option set (the parent's library)"""
    import design_ref as dref
    from magnetite_amd import Context, meshgen
    from magnetite_amd._lib import MAG_STOP_REL
    prob = dref.cantilever(meshgen.baseline_problem("plate100k").mesh)
    opts = dict(device=0, stop_mode=MAG_STOP_REL, tol=tol)
    if kind is not None:
        opts["field_cg"] = kind
    rows, solved_scale = [], None
    with Context(**opts) as c:
        c.upload_problem(prob)
        c.design_init(volume_fraction=0.5)
        for it in range(ITERS):
            if it == ITERS - 1:
                solved_scale = c.download_design()["scale"]
            t0 = time.perf_counter()
            c.run()
            c.run_sensitivities("run")
            t1 = time.perf_counter()
            c.design_step()
            t2 = time.perf_counter()
            st = c.stats()
            rows.append({"iteration": it, "cg_iterations": st["iterations"], "cg_kernel": st["cg_kernel"], "ms_cg": round(st["ms_cg"], 4),
                         "us_per_cg_iteration": round(1e3 * st["ms_cg"] / max(st["iterations"], 1), 4),
                         "ms_assemble": round(st["ms_assemble"], 4), "ms_order": round(st["ms_order"], 4),
                         "ms_csr_symbolic": round(st["ms_csr_symbolic"], 4), "wall_ms": round((t2 - t0) * 1e3, 3),
                         "design_step_ms": round((t2 - t1) * 1e3, 4), "J": c.design_info()["J"]})
    wall, ms_cg, us, its = [], [], [], []
    with Context(**opts) as c:
        c.upload_problem(prob)
        c.set_element_scale(solved_scale)
        c.run()  # (order, pattern, table, graph)
        c.run_sensitivities("run")
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            c.run()
            c.run_sensitivities("run")
            wall.append((time.perf_counter() - t0) * 1e3)
            st = c.stats()
            ms_cg.append(st["ms_cg"])
            us.append(1e3 * st["ms_cg"] / max(st["iterations"], 1))
            its.append(st["iterations"])
    assert len(set(its)) == 1, its
    return {"field_cg": kind, "iterations": rows,
            "design_of_iteration_20": {"cg_iterations": its[0], "cg_kernel": st["cg_kernel"], "wall_ms": summary(wall), "ms_cg": summary(ms_cg),
                                       "us_per_cg_iteration": summary(us)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_cg.json"))
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--leg", default=None, help="(internal) run one leg and print it as JSON: parent | 0 | 1 | 2 | 3")
    a = ap.parse_args()
    if a.leg is not None:
        print("LEG " + json.dumps(leg(None if a.leg == "parent" else int(a.leg), a.tol)))
        return

    def child(which, lib=None):
        env = dict(os.environ)
        if lib:
            env["MAG_LIB_PATH"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--tol", str(a.tol)], env=env, capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"leg {which} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1][4:])

    if not a.parent_lib:
        raise SystemExit("--parent-lib is needed: the yardstick is the parent commit's library in the same session")
    out = {"mesh": "plate100k", "cg_tol_rel": a.tol, "design_iterations": ITERS, "volume_fraction": 0.5, "repeats": REPEATS,
           "parent": child("parent", a.parent_lib), "legs": {}}
    for kind in (0, 1, 2, 3):
        out["legs"][str(kind)] = child(str(kind))
        print("field_cg", kind, json.dumps(out["legs"][str(kind)]["design_of_iteration_20"]), flush=True)
    par, legs = out["parent"], out["legs"]
    counts = lambda L: [r["cg_iterations"] for r in L["iterations"]]
    out["like_for_like"] = counts(par) == counts(legs["0"])
    p20 = par["design_of_iteration_20"]
    spread_us = p20["us_per_cg_iteration"]["max"] - p20["us_per_cg_iteration"]["min"]
    spread_wall = p20["wall_ms"]["max"] - p20["wall_ms"]["min"]
    best = min(("1", "2", "3"), key=lambda k: legs[k]["design_of_iteration_20"]["wall_ms"]["median"])
    base0 = legs["0"]["iterations"]
    out["table_build_ms"] = {k: round(legs[k]["iterations"][0]["ms_csr_symbolic"] - base0[0]["ms_csr_symbolic"], 4) for k in ("1", "2", "3")}
    out["gather_and_inverse_blocks_ms_per_assembly"] = {
        k: round(statistics.median(r["ms_assemble"] - b["ms_assemble"] for r, b in zip(legs[k]["iterations"][1:], base0[1:])), 4) for k in ("1", "2", "3")}
    out["requirements"] = {
        "parent_us_per_cg_iteration": p20["us_per_cg_iteration"], "field_cg_1_us_per_cg_iteration": legs["1"]["design_of_iteration_20"]["us_per_cg_iteration"],
        "us_per_cg_iteration_met": legs["1"]["design_of_iteration_20"]["us_per_cg_iteration"]["median"] < p20["us_per_cg_iteration"]["median"] - spread_us,
        "best_field_cg": int(best), "parent_wall_ms": p20["wall_ms"], "best_wall_ms": legs[best]["design_of_iteration_20"]["wall_ms"],
        "whole_iteration_met": legs[best]["design_of_iteration_20"]["wall_ms"]["median"] < p20["wall_ms"]["median"] - spread_wall}
    print(json.dumps({k: out[k] for k in ("like_for_like", "table_build_ms", "gather_and_inverse_blocks_ms_per_assembly", "requirements")}))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if not out["like_for_like"]:
        raise SystemExit("the new build's field_cg = 0 leg does not reproduce the parent's iteration counts")


if __name__ == "__main__":
    main()
