"""Context.objective(kind, "variants", adjoint=True) against the route a user had before it, on the same context: download u of
every variant, the objective, dJ/du and the explicit partials in numpy (tests/objective_ref.py in float64), Context.adjoint(g),
and the sum of the two parts on the host.

Two sizes: 64 variants of the tensile fixture, 42 of the 3k-node holes mesh; both objectives, weights scaled so that |dJ/du|
matches the right-hand side.  The primal solves are done once and are not timed.  After a warm-up, five repeats each, median and
spread (max - min).
    python scripts/objective_probe.py [--out profiles/objective.json]"""
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
REPEATS = 5
SIZES = (("tensile", 64), ("holes3k", 42))
KINDS = ("stress_pnorm", "disp_lsq")


def med(v):
    return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "repeats": len(v)}


def timed(fn):
    fn()  # warm-up
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return med(times), out


def row(prob, name, V, kind):
    import adjoint_ref as aref
    import objective_ref as oref
    from magnetite_amd import Context
    from variants_util import make_variants
    xy, mat, u, f = make_variants(prob, V, seed=11)
    free = prob.u_known == 0
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        if kind == "stress_pnorm":
            sig = oref.element_stress(np.asarray(prob.mesh.xy).reshape(-1, 2), np.asarray(prob.mesh.conn).reshape(-1, 3), outs[0]["u"], prob.poisson_ratio, prob.youngs_modulus)
            spec = dict(weights=np.ones(prob.mesh.num_elements), p=8.0, scale=float(np.sqrt(oref.von_mises_sq(sig)).max()))
        else:
            spec = dict(weights=aref.patch_weights(prob), target=0.5 * outs[0]["u"])
        first = c.objective(kind, "variants", **spec)
        factors = np.array([o["rhs_norm"] / np.linalg.norm(g["g"][free]) for o, g in zip(outs, first)]) ** spec.get("p", 1.0)
        spec["weights"] = np.ascontiguousarray(spec["weights"][None, :] * factors[:, None])
        if "target" in spec:
            spec["target"] = np.ascontiguousarray(np.broadcast_to(spec["target"], spec["weights"].shape))

        def legacy():
            parts = [oref.of_problem(kind, prob, c.download_variant(i)[0], xy[i], mat[i], ext=False,
                                     **{k: (v[i] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in spec.items()})
                     for i in range(V)]
            adj = c.adjoint(np.stack([p["g"] for p in parts]), "variants")
            return [p["pxy"] + a["dxy"] for p, a in zip(parts, adj)]

        t_new, new = timed(lambda: c.objective(kind, "variants", adjoint=True, **spec))
        t_old, old = timed(legacy)
    out = {"mesh": name, "variants": V, "kind": kind, "objective_with_adjoint": t_new, "download_numpy_adjoint": t_old,
           "rel_dxy_between_legs": float(np.linalg.norm(new[-1]["dxy"] - old[-1]) / np.linalg.norm(old[-1])),
           "speedup": round(t_old["median_ms"] / t_new["median_ms"], 2)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective.json"))
    a = ap.parse_args()
    from load_cases_probe import problems
    probs = problems()
    rows = [row(probs[name], name, V, kind) for name, V in SIZES for kind in KINDS]
    with open(a.out, "w") as fh:
        json.dump({"repeats": REPEATS, "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
