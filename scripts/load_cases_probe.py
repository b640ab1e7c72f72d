"""Load cases against the same cases solved one after another (mag_set_load_cases / mag_run_cases).

For plate(16), the 3k-node holes mesh, the tensile fixture and plate100k, with L = floor(CUs / G) and 4 floor(CUs / G) cases
(G: the workgroups one case needs), after a warm-up, five repeats each, median and spread (max - min):
  (a) run_cases: wall time, and the HIP-event time of its on-chip CG launches (ms_cg per launch, summed);
  (b) the same L cases as upload + run + download, one after another on one warm context -- the existing API only.
Leg (b) is the baseline and belongs to the commit BEFORE load cases existed: check that commit out somewhere, build it, and
pass the checkout with --baseline-tree (its package and library are then imported by the child process that runs leg (b));
without the option (b) runs on the current tree.
Per-iteration time of a full chunk (L = floor(CUs / G): one launch) against the single case's ms_cg / iterations of leg (b).
    python scripts/load_cases_probe.py [--baseline-tree DIR] [--out profiles/load_cases.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MAG_PROBE_PACKAGE_ROOT") or ROOT)  # (leg (b): the baseline checkout's magnetite_amd)
sys.path.insert(1, os.path.join(ROOT, "tests"))
REPEATS = 5


def problems():
    from magnetite_amd import meshgen
    g = np.load(os.path.join(ROOT, "tests", "golden", "tensile.npz"))
    tensile = meshgen.Problem(meshgen.Mesh(g["xy"], g["conn"].astype(np.int32), "tensile"), g["u_known"].astype(np.uint8), g["u_in"],
                              g["f_in"], *[float(v) for v in g["material"]])
    return {"plate16": meshgen.config_fixed_left_pull_right(meshgen.plate(16)),
            "holes3k": meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3)),
            "tensile": tensile,
            "plate100k": meshgen.baseline_problem("plate100k")}


def med(v):
    return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "repeats": len(v)}


def cases_for(prob, L):
    from load_cases_util import make_cases
    u, f = make_cases(prob, L, seed=11)
    u[1], f[1] = u[0], f[0]  # (no 1e-3 x case here: every case of a chunk runs about as long as a single solve)
    return u, f


def leg_sequential(names_L):
    """(b): existing API only.  Returns {name: {L: stats}} and the single-case per-iteration time."""
    from load_cases_util import case_problem
    from magnetite_amd import Context
    out = {}
    probs = problems()
    for name, Ls in names_L.items():
        prob = probs[name]
        out[name] = {}
        for L in Ls:
            u, f = cases_for(prob, L)
            cps = [case_problem(prob, u[i], f[i]) for i in range(L)]
            with Context(device=0) as c:
                c.solve(cps[0])  # warm-up
                walls, per_it = [], []
                for _ in range(REPEATS):
                    t0 = time.perf_counter()
                    for cp in cps:
                        c.upload_problem(cp)
                        c.run()
                        c.download()
                    walls.append((time.perf_counter() - t0) * 1e3)
                    st = c.stats()
                    per_it.append(st["ms_cg"] * 1e3 / max(1, st["iterations"]))
            out[name][str(L)] = {"wall": med(walls), "single_case_us_per_iteration": round(statistics.median(per_it), 3)}
    return out


def leg_cases(names_L):
    from magnetite_amd import Context
    out = {}
    probs = problems()
    for name, Ls in names_L.items():
        prob = probs[name]
        out[name] = {}
        for L in Ls:
            u, f = cases_for(prob, L)
            with Context(device=0) as c:
                c.upload_problem(prob)
                c.set_load_cases(u, f)
                c.run_cases()  # warm-up
                walls, launches, per_it = [], [], []
                for _ in range(REPEATS):
                    t0 = time.perf_counter()
                    c.run_cases()
                    for i in range(L):
                        c.download_case(i)
                    walls.append((time.perf_counter() - t0) * 1e3)
                    info = c.cases_info()
                    sts = [c.case_stats(i) for i in range(L)]
                    first = sts[::max(1, info["cases_per_launch"])]  # one case per launch
                    launches.append(sum(s["ms_cg"] for s in first))
                    per_it.append(sts[0]["ms_cg"] * 1e3 / max(1, max(s["iterations"] for s in sts[:max(1, info["cases_per_launch"])])))
            out[name][str(L)] = {"info": info, "wall": med(walls), "cg_launches": med(launches),
                                 "first_chunk_us_per_iteration": round(statistics.median(per_it), 3)}
    return out


def shapes():
    """{name: [floor(CUs / G), 4 floor(CUs / G)]} from one single-case solve each and the device's CU count."""
    from magnetite_amd import Context
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, check=True)
    cus = int(r.stdout.split()[-1])
    out = {}
    for name, prob in problems().items():
        with Context(device=0) as c:
            st = c.solve(prob)
        G = -(-st["num_tiles"] // max(1, st["tiles_per_workgroup"]))
        n = max(1, cus // G)
        out[name] = [n, 4 * n]
    return cus, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "load_cases.json"))
    ap.add_argument("--leg", choices=("sequential",), help=argparse.SUPPRESS)
    ap.add_argument("--shapes", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == "sequential":  # child process: the package of MAG_PROBE_PACKAGE_ROOT
        print("RESULT " + json.dumps(leg_sequential(json.loads(a.shapes))), flush=True)
        return
    cus, names_L = shapes()
    env = dict(os.environ)
    if a.baseline_tree:
        env["MAG_PROBE_PACKAGE_ROOT"] = os.path.abspath(a.baseline_tree)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "sequential", "--shapes", json.dumps(names_L)], env=env,
                       capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit("sequential leg failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    seq = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    cases = leg_cases(names_L)
    rows = []
    for name, Ls in names_L.items():
        for L in Ls:
            b, c = seq[name][str(L)], cases[name][str(L)]
            rows.append({"mesh": name, "cases": L, "run_cases": c, "sequential": b,
                         "speedup": round(b["wall"]["median_ms"] / c["wall"]["median_ms"], 3),
                         "faster_by_more_than_the_spread": b["wall"]["median_ms"] - c["wall"]["median_ms"] > b["wall"]["spread_ms"],
                         "chunk_over_single_per_iteration": round(c["first_chunk_us_per_iteration"] / b["single_case_us_per_iteration"], 3)})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"compute_units": cus, "baseline_library": "the parent commit's build" if a.baseline_tree else "this build",
           "repeats": REPEATS, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
