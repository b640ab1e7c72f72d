"""mag_run_refine against what a user does today with the same marks -- the mesh on the host, the refinement in numpy (the
vectorised twin, tests/refine_ref.py) -- and against mag_run of the same mesh for scale.

Two meshes: the 100k-triangle plate and the 1M-triangle plate with a hole (the baseline's problems), 20 % of the elements marked:
by explicit marks (the fifth of the elements nearest a point, a patch as an error indicator produces it) and by top-fraction of a
caller's indicator (the distance to that point, negated and shifted: the same elements through the check, the keys and the sort).
After a warm-up, REPEATS repeats each, the legs alternating, median and spread (max - min) of the host's wall time -- every call
ends in a device synchronise:
  (a) run_refine by marks, by indicator (with its upload of E doubles), and with download_refine of every array;
  (b) upload_refined, device to device;
  (c) the numpy twin on the host arrays;
  (d) run() of the coarse mesh: ms_total of its statistics and the host's wall time.
The file also holds the compulsory bytes of the pass (read conn three times and the tables it builds once, write the refined
mesh) over the wall time of run_refine as a fraction of the HBM peak -- of the call, with its launches, two sorts, three scans
and its read-backs, not of a kernel.  The arrays of (a) are compared with (c)'s: equal or the probe fails.
    python scripts/refine_probe.py [--out profiles/refine.json]"""
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
HBM_PEAK = 8e12  # bytes per second
ARRAYS = ("xy", "conn", "u_known", "u_in", "f_in", "node_parents", "elem_parent")


def med(v):
    return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "repeats": len(v)}


def measure(ctx, prob):
    import refine_ref as ref
    xy, conn = prob.mesh.xy, prob.mesh.conn
    E, N = len(conn), len(xy)
    c = xy[conn].mean(axis=1)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    dist = np.hypot(*(c - (lo + 0.37 * (hi - lo))).T)
    indicator = dist.max() - dist
    k = int(np.ceil(0.2 * E))
    marks = np.zeros(E, dtype=np.uint8)
    marks[np.argsort(-indicator, kind="stable")[:k]] = 1
    ctx.run_refine(marks=marks)  # warm-up
    ctx.run_refine(indicator=indicator, rule="top_fraction", theta=0.2)
    ctx.download_refine()
    legs = {k: [] for k in ("run_refine_marks", "run_refine_indicator", "refine_with_download", "numpy_twin")}
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        ctx.run_refine(marks=marks)
        t1 = time.perf_counter()
        ctx.run_refine(indicator=indicator, rule="top_fraction", theta=0.2)
        t2 = time.perf_counter()
        ctx.run_refine(marks=marks)
        got = ctx.download_refine()
        t3 = time.perf_counter()
        want = ref.of_problem(prob, marks=marks)
        t4 = time.perf_counter()
        for name, dt in zip(legs, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            legs[name].append(dt * 1e3)
    for name in ARRAYS:
        assert got[name].tobytes() == want[name].tobytes(), name
    info = ctx.refine_info()
    out = {name: med(v) for name, v in legs.items()}
    out.update(refined_nodes=info["nodes"], refined_elements=info["elements"], marked=info["marked"], sweeps=info["sweeps"])
    m = {name: statistics.median(v) for name, v in legs.items()}
    out["speedup_with_download_over_numpy"] = round(m["numpy_twin"] / m["refine_with_download"], 2)
    # the solve of the same mesh, for scale; then the upload of the refined one
    solve = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.run()
        solve.append((time.perf_counter() - t0) * 1e3)
    st = ctx.stats()
    out["run_wall"] = med(solve)
    out["run_ms_total"] = round(st["ms_total"], 4)
    out["run_iterations"] = st["iterations"]
    out["run_refine_over_run"] = round(m["run_refine_marks"] / statistics.median(solve), 5)
    up = []
    for _ in range(REPEATS):
        ctx.run_refine(marks=marks)
        t0 = time.perf_counter()
        ctx.upload_refined()
        up.append((time.perf_counter() - t0) * 1e3)
        ctx.upload_problem(prob)
    out["upload_refined"] = med(up)
    Nn, En = info["nodes"], info["elements"]
    # conn read by the key, longest-edge and emission kernels; keys and slots written, sorted (read + written once per pass is
    # the sort's own business: counted once each way), heads, scan, edge ids, edge keys, flags and their scan, counts and
    # their scan; the refined mesh written, the old nodes' rows copied
    out["compulsory_bytes"] = 3 * 12 * E + 2 * (12 * 3 * E) + 3 * (4 * 3 * E) + 8 * 3 * E + 2 * (4 * 3 * E) + 2 * 4 * E + (16 + 2 + 32) * (Nn + N) + 16 * En
    out["hbm_peak_fraction_of"] = "wall time of mag_run_refine (marks)"
    out["hbm_peak_fraction"] = round(out["compulsory_bytes"] / (m["run_refine_marks"] * 1e-3) / HBM_PEAK, 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine.json"))
    a = ap.parse_args()
    from magnetite_amd import Context, meshgen
    rows = []
    for name in ("plate100k", "hole1m"):
        prob = meshgen.baseline_problem(name)
        with Context(device=0) as c:
            c.upload_problem(prob)
            row = {"mesh": name, "nodes": prob.mesh.num_nodes, "elements": prob.mesh.num_elements}
            row.update(measure(c, prob))
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"repeats": REPEATS, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
