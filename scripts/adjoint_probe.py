"""Context.adjoint("cases") against the route a user had before it, on the PARENT commit's library: solve_cases for the adjoint
systems (which drops nothing the user still needs only because the primal results were downloaded first), download of u and
lambda, and the numpy statement of the bilinear pass in tests/adjoint_ref.py per member.

Two sizes: 64 load cases of the tensile fixture, 42 of the 3k-node holes mesh; the objective is J = sum w u^2 over a node patch,
w scaled so that |dJ/du| matches the right-hand side.  The primal solves are done once and are not timed.  After a warm-up, five
repeats each, median and spread (max - min).  The legacy leg runs in a child process with MAG_LIB_PATH set to --parent-lib, a
build of the parent commit's csrc/; without --parent-lib it runs on this build (the calls it makes are the same) and the file
says so.
    python scripts/adjoint_probe.py [--parent-lib /path/to/libmagnetite_hip.so] [--out profiles/adjoint.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.join(ROOT, "scripts"))
REPEATS = 5
SIZES = (("tensile", 64), ("holes3k", 42))


def med(v):
    return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "repeats": len(v)}


def setup(name, L):
    """The problem, its load sets, the primal solutions and dJ/du per case (through whichever library this process loaded)."""
    import adjoint_ref as aref
    from load_cases_probe import problems
    from load_cases_util import make_cases
    from magnetite_amd import Context
    prob = problems()[name]
    u, f = make_cases(prob, L, seed=11)
    c = Context(device=0)
    outs = c.solve_cases(prob, u, f)
    w0 = aref.patch_weights(prob)
    G = np.stack([aref.dJ1(w0 * (o["rhs_norm"] / np.linalg.norm(aref.dJ1(w0, o["u"])[prob.u_known == 0])), o["u"]) for o in outs])
    return prob, u, f, c, [o["u"] for o in outs], G


def leg_adjoint(name, L):
    prob, u, f, c, U, G = setup(name, L)
    c.adjoint(G, "cases")  # warm-up
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        outs = c.adjoint(G, "cases")
        times.append((time.perf_counter() - t0) * 1e3)
    c.close()
    return {"adjoint_cases_with_downloads": med(times), "dxy_norm_last": float(np.linalg.norm(outs[-1]["dxy"]))}


def leg_legacy(name, L):
    import adjoint_ref as aref
    prob, u, f, c, U, G = setup(name, L)
    mat = (prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)

    def route():
        adj = c.solve_cases(prob, np.zeros_like(G), G)  # (the primal cases' results are gone from the context now)
        return [aref.adjoint(prob.mesh.xy, prob.mesh.conn, prob.u_known, U[i], adj[i]["u"], G[i], adj[i]["f"], *mat) for i in range(L)]

    route()  # warm-up
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        outs = route()
        times.append((time.perf_counter() - t0) * 1e3)
    c.close()
    return {"solve_cases_download_numpy": med(times), "dxy_norm_last": float(np.linalg.norm(outs[-1]["dxy"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjoint.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--leg", choices=("adjoint", "legacy"), default=None)
    a = ap.parse_args()
    if a.leg:  # a child: one leg, every size, one JSON line
        print(json.dumps([(leg_adjoint if a.leg == "adjoint" else leg_legacy)(name, L) for name, L in SIZES]), flush=True)
        return
    legs = {}
    for leg in ("adjoint", "legacy"):  # a process per leg: the library is chosen when the binding is imported
        env = dict(os.environ)
        if leg == "legacy" and a.parent_lib:
            env["MAG_LIB_PATH"] = os.path.abspath(a.parent_lib)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], env=env, capture_output=True, text=True, timeout=1500)
        if out.returncode != 0:
            sys.exit(f"leg {leg} failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
        legs[leg] = json.loads(out.stdout.strip().splitlines()[-1])
    rows = []
    for k, (name, L) in enumerate(SIZES):
        row = {"mesh": name, "cases": L}
        row.update(legs["adjoint"][k])
        new_norm = row.pop("dxy_norm_last")
        row.update(legs["legacy"][k])
        row["rel_dxy_norm_between_legs"] = abs(row.pop("dxy_norm_last") - new_norm) / new_norm
        row["speedup"] = round(row["solve_cases_download_numpy"]["median_ms"] / row["adjoint_cases_with_downloads"]["median_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"repeats": REPEATS, "legacy_library": "parent commit (MAG_LIB_PATH)" if a.parent_lib else "this build", "rows": rows},
                  fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
