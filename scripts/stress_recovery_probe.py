"""mag_run_stress against what a user does today on the same solved outputs -- download every member's u, then the recovery in
numpy (tests/stress_recovery_ref.py) -- and against mag_run_sensitivities on the same context, a pass of about the same traffic.

Two sizes: 42 variants of the 3k-node holes mesh and 8 variants of the 100k-triangle plate (shape, material and loads varied).
The solves are done once and are not timed.  After a warm-up, REPEATS repeats each, the three legs alternating, median and
spread (max - min) of the host's wall time (each call ends in a device synchronise):
  (a) run_stress alone, and with the downloads of every member's rows;
  (b) run_sensitivities alone, and with its downloads;
  (c) per member: download u, then the numpy reference.
Per member the pass reads conn (12 E bytes) and the coordinates and u (32 N), and writes 40 E + 32 N bytes of results; the
file holds those compulsory bytes over the wall time of run_stress as a fraction of the HBM peak (8 TB/s) -- of the call, with its
five launches per chunk and the copy of the scalars, not of a kernel.
    python scripts/stress_recovery_probe.py [--out profiles/stress_recovery.json]"""
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
sys.path.insert(2, os.path.join(ROOT, "scripts"))
REPEATS = 7
HBM_PEAK = 8e12  # bytes per second


def med(v):
    return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "repeats": len(v)}


def measure(ctx, prob, V, xy, mat):
    import stress_recovery_ref as ref
    ctx.run_stress("variants")  # warm-up
    ctx.run_sensitivities("variants")
    legs = {k: [] for k in ("run_stress", "stress_with_downloads", "run_sensitivities", "sensitivities_with_downloads", "download_u_and_numpy")}
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        ctx.run_stress("variants")
        t1 = time.perf_counter()
        fields = [ctx.download_stress("variants", i) for i in range(V)]
        t2 = time.perf_counter()
        ctx.run_sensitivities("variants")
        t3 = time.perf_counter()
        [ctx.download_sensitivity("variants", i) for i in range(V)]
        t4 = time.perf_counter()
        for i in range(V):
            u = ctx.download_variant(i)[0]
            want = ref.stress_recovery(xy[i], prob.mesh.conn, u, *mat[i])
        t5 = time.perf_counter()
        for k, dt in zip(legs, (t1 - t0, t2 - t0, t3 - t2, t4 - t2, t5 - t4)):
            legs[k].append(dt * 1e3)
    out = {k: med(v) for k, v in legs.items()}
    m = {k: statistics.median(v) for k, v in legs.items()}
    out["speedup_with_downloads_over_numpy"] = round(m["download_u_and_numpy"] / m["stress_with_downloads"], 2)
    out["run_stress_over_run_sensitivities"] = round(m["run_stress"] / m["run_sensitivities"], 3)
    # the legs computed the same thing (last member)
    out["rel_eta2_between_legs"] = float(np.linalg.norm(want["eta2"] - fields[-1]["eta2"]) / np.linalg.norm(want["eta2"]))
    out["rel_node_between_legs"] = float(np.linalg.norm(want["node"] - fields[-1]["node"]) / np.linalg.norm(want["node"]))
    N, E = prob.mesh.num_nodes, prob.mesh.num_elements
    out["compulsory_bytes"] = V * ((12 * E + 32 * N) + (40 * E + 32 * N))
    out["hbm_peak_fraction_of"] = "wall time of mag_run_stress"
    out["hbm_peak_fraction"] = round(out["compulsory_bytes"] / (m["run_stress"] * 1e-3) / HBM_PEAK, 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stress_recovery.json"))
    a = ap.parse_args()
    from magnetite_amd import Context, meshgen
    from variants_util import make_variants
    rows = []
    for name, make, V in (("holes3k", lambda: meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3)), 42),
                          ("plate100k", lambda: meshgen.baseline_problem("plate100k"), 8)):
        prob = make()
        xy, mat, u, f = make_variants(prob, V, seed=11)
        with Context(device=0) as c:
            c.upload_problem(prob)
            c.set_variants(xy, mat, u, f)
            c.run_variants()
            row = {"mesh": name, "nodes": prob.mesh.num_nodes, "elements": prob.mesh.num_elements, "variants": V}
            row.update(measure(c, prob, V, xy, mat))
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"repeats": REPEATS, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
