"""mag_run_sensitivities against what a user does today on the same solved outputs: download u, then the element loop in numpy.

Three sizes: 256 variants of the tensile fixture, 42 variants of the 3k-node holes mesh (shape, material and loads varied), one
run of the 1M-triangle holes mesh.  The solves are done once and are not timed.  After a warm-up, five repeats each, median
and spread (max - min):
  (a) run_sensitivities alone (the library's call; it waits for the device), and with the downloads of every member;
  (b) per member: download u, then numpy -- element energies, the node gradient by the closed form gathered with np.add.at,
      the scalars (the vectorised loop a user would write; the per-element Python loop is slower still).
At 1M triangles the file also holds the fraction of the HBM peak (8 TB/s) in compulsory bytes, 32N + 12E read and 16N + 8E
written per member.
    python scripts/sensitivities_probe.py [--out profiles/sensitivities.json]"""
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
HBM_PEAK = 8e12  # bytes per second


def med(v):
    return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "repeats": len(v)}


def numpy_loop(xy, conn, u_known, u, f, u_in, f_in, youngs, nu, t):
    """energy, dxy and the scalars from downloaded arrays: the closed form, vectorised over the elements."""
    p, d = xy.reshape(-1, 2)[conn], u.reshape(-1, 2)[conn]
    x, y, ux, uy = p[..., 0], p[..., 1], d[..., 0], d[..., 1]
    r1, r2 = np.roll(np.arange(3), -1), np.roll(np.arange(3), -2)
    b, g = y[:, r1] - y[:, r2], x[:, r2] - x[:, r1]
    P, Q_, R = (b * ux).sum(1), (g * uy).sum(1), (g * ux + b * uy).sum(1)
    A2 = (x * b).sum(1)
    Q = P * P + Q_ * Q_ + 2 * nu * P * Q_ + 0.5 * (1 - nu) * R * R
    cm = youngs * t / (4 * (1 - nu * nu))
    energy = cm * Q / A2
    dxy = np.zeros(xy.size)
    for m in range(3):
        m1, m2 = (m + 1) % 3, (m + 2) % 3
        dQx = 2 * (Q_ + nu * P) * (uy[:, m1] - uy[:, m2]) + (1 - nu) * R * (ux[:, m1] - ux[:, m2])
        dQy = 2 * (P + nu * Q_) * (ux[:, m2] - ux[:, m1]) + (1 - nu) * R * (uy[:, m2] - uy[:, m1])
        np.add.at(dxy, 2 * conn[:, m], cm / A2 * (dQx - Q * b[:, m] / A2))
        np.add.at(dxy, 2 * conn[:, m] + 1, cm / A2 * (dQy - Q * g[:, m] / A2))
    om = 1 - nu * nu
    dnu = (youngs * t / (4 * A2) * ((2 * P * Q_ - 0.5 * R * R) / om + 2 * nu * Q / om ** 2)).sum()
    free = u_known == 0
    W, ext = energy.sum(), (f_in[free] * u[free]).sum()
    return energy, dxy, (W, W - ext, ext, (f[~free] * u_in[~free]).sum(), W / youngs, dnu, W / t)


def measure(ctx, set_name, members, numpy_args):
    ctx.run_sensitivities(set_name)  # warm-up
    alone, with_dl, host = [], [], []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        ctx.run_sensitivities(set_name)
        t1 = time.perf_counter()
        outs = [ctx.download_sensitivity(set_name, i) for i in range(members)]
        t2 = time.perf_counter()
        alone.append((t1 - t0) * 1e3)
        with_dl.append((t2 - t0) * 1e3)
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for i in range(members):
            args = numpy_args(i)
            res = numpy_loop(*args)
        host.append((time.perf_counter() - t0) * 1e3)
    # the two legs computed the same thing (last member)
    agree = float(np.linalg.norm(res[1] - outs[-1]["dxy"]) / np.linalg.norm(outs[-1]["dxy"]))
    return {"run_sensitivities": med(alone), "with_downloads": med(with_dl), "download_u_and_numpy": med(host),
            "speedup_with_downloads": round(statistics.median(host) / statistics.median(with_dl), 2), "rel_dxy_between_legs": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivities.json"))
    a = ap.parse_args()
    from load_cases_probe import problems
    from magnetite_amd import Context, meshgen
    from variants_util import make_variants
    probs = problems()
    rows = []
    for name, V in (("tensile", 256), ("holes3k", 42)):
        prob = probs[name]
        xy, mat, u, f = make_variants(prob, V, seed=11)
        with Context(device=0) as c:
            c.upload_problem(prob)
            c.set_variants(xy, mat, u, f)
            c.run_variants()

            def args(i):
                ui, fi, _ = c.download_variant(i)
                return xy[i], prob.mesh.conn, prob.u_known, ui, fi, u[i], f[i], mat[i][0], mat[i][1], mat[i][2]

            row = {"mesh": name, "nodes": prob.mesh.num_nodes, "elements": prob.mesh.num_elements, "variants": V}
            row.update(measure(c, "variants", V, args))
        rows.append(row)
        print(json.dumps(row), flush=True)
    prob = meshgen.baseline_problem("hole1m")
    N, E = prob.mesh.num_nodes, prob.mesh.num_elements
    with Context(device=0) as c:
        c.solve(prob)

        def args1(i):
            ui, fi, _ = c.download()
            return (prob.xy_flat, prob.mesh.conn, prob.u_known, ui, fi, prob.u_in, prob.f_in, prob.youngs_modulus,
                    prob.poisson_ratio, prob.part_thickness)

        row = {"mesh": "hole1m", "nodes": N, "elements": E, "variants": 1}
        row.update(measure(c, "run", 1, args1))
    compulsory = (32 * N + 12 * E) + (16 * N + 8 * E)
    row["compulsory_bytes"] = compulsory
    # (of the host's wall time of the call: four launches, the copy of the scalars and a stream synchronise, and the traffic that
    # is not compulsory -- not kernel time)
    row["hbm_peak_fraction_of"] = "wall time of mag_run_sensitivities"
    row["hbm_peak_fraction"] = round(compulsory / (row["run_sensitivities"]["median_ms"] * 1e-3) / HBM_PEAK, 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"repeats": REPEATS, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
