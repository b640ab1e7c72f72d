"""mag_design_step against what a user does without it on the same library -- download the energies, take the design step in
numpy (the twin, tests/design_ref.py), hand the new scale back with set_element_scale -- and one whole design iteration
(run + run_sensitivities + step) of both kinds, on the 100k-triangle plate under a point load.

After a warm-up of two iterations, REPEATS iterations each, the device's and the host's legs alternating on two contexts that
hold the same design, median and spread (max - min) of the host's wall time -- every call ends in a device synchronise:
  (a) design_step on the device-resident energies;
  (b) download_sensitivity + the twin's step + set_element_scale;
  (c), (d) the whole iteration around (a) and around (b): run, run_sensitivities, the step;
and of the iteration's run() its ms_total, ms_assemble, ms_cg and CG iterations, ms_order and ms_csr_symbolic (0 after the first).
The densities of the two contexts are compared after every iteration.  One step from the same energies differs by the order
of the volume sum only (tests/test_design_gpu.py); over iterations the two designs, each re-solved to the CG tolerance, drift
apart by that tolerance's effect on the energies: the largest difference is recorded, and beyond 1e3 x tol the probe fails.
    python scripts/design_probe.py [--out profiles/design.json]"""
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
WARMUP = 2


def med(v):
    return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "design.json"))
    ap.add_argument("--tol", type=float, default=1e-8)
    a = ap.parse_args()
    import design_ref as dref
    from magnetite_amd import Context, meshgen
    from magnetite_amd._lib import MAG_STOP_REL
    prob = dref.cantilever(meshgen.baseline_problem("plate100k").mesh)
    legs = {k: [] for k in ("design_step", "host_step", "iteration_device", "iteration_host")}
    runs, worst = [], 0.0
    with Context(device=0, stop_mode=MAG_STOP_REL, tol=a.tol) as dev, Context(device=0, stop_mode=MAG_STOP_REL, tol=a.tol) as host:
        dev.upload_problem(prob)
        dev.design_init()
        host.upload_problem(prob)
        twin = dref.Design(prob.mesh.xy, prob.mesh.conn)
        host.set_element_scale(twin.scale)
        for it in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            dev.run()
            dev.run_sensitivities("run")
            t1 = time.perf_counter()
            dev.design_step()
            t2 = time.perf_counter()
            st = dev.stats()
            t3 = time.perf_counter()
            host.run()
            host.run_sensitivities("run")
            t4 = time.perf_counter()
            energy = host.download_sensitivity("run", 0)["energy"]
            twin.step(energy=energy)
            host.set_element_scale(twin.scale)
            t5 = time.perf_counter()
            diff = float(np.abs(dev.download_design()["rho"] - twin.rho).max())
            assert diff <= 1e3 * a.tol, (it, diff)
            worst = max(worst, diff)
            if it >= WARMUP:
                for name, dt in zip(legs, (t2 - t1, t5 - t4, t2 - t0, t5 - t3)):
                    legs[name].append(dt * 1e3)
                runs.append(st)
        info = dev.design_info()
    out = {"mesh": "plate100k", "nodes": prob.mesh.num_nodes, "elements": prob.mesh.num_elements, "cg_tol_rel": a.tol, "warmup": WARMUP}
    out.update({name: med(v) for name, v in legs.items()})
    m = {name: statistics.median(v) for name, v in legs.items()}
    out["step_speedup_over_host"] = round(m["host_step"] / m["design_step"], 2)
    out["iteration_speedup_over_host"] = round(m["iteration_host"] / m["iteration_device"], 3)
    for key in ("ms_total", "ms_order", "ms_csr_symbolic", "ms_assemble", "ms_cg"):
        out["run_" + key] = med([r[key] for r in runs])
    out["run_iterations"] = [int(r["iterations"]) for r in runs]
    out["run_cg_kernel"] = sorted({int(r["cg_kernel"]) for r in runs})
    out["largest_density_difference_device_host"] = worst
    out["design_after"] = {k: info[k] for k in ("volume_fraction", "change", "greyness", "J", "steps")}
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
