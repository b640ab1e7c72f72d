"""Design variants against the same variants solved one after another (mag_set_variants / mag_run_variants).

Three sizes: 256 variants of the tensile fixture, floor(CUs / G) + 3 variants of the 3k-node holes mesh, 2 variants of
plate100k -- shape (a morph of at most 0.2 shortest edges), material and loads all varied.  After a warm-up, five repeats
each, median and spread (max - min):
  (a) solve_variants: wall time with the downloads, and the phases mag_get_variant_stats reports for a side-by-side run
      (permute = ms_element, assemble, right-hand sides + blocks = ms_bc, CG launches = ms_cg summed per launch, post);
  (b) the same variants as upload + run + download, one after another on one warm context -- the existing API only.
Leg (b) belongs to the commit BEFORE variants existed: check that commit out somewhere, build it, and pass the checkout with
--baseline-tree (its package and library are imported by the child process that runs leg (b)); without the option (b) runs
on the current tree.
    python scripts/variants_probe.py [--baseline-tree DIR] [--out profiles/variants.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MAG_PROBE_PACKAGE_ROOT") or ROOT)  # (leg (b): the baseline checkout's magnetite_amd)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.join(ROOT, "scripts"))
REPEATS = 5


def med(v):
    return {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "repeats": len(v)}


def problems():
    from load_cases_probe import problems as base
    p = base()
    return {k: p[k] for k in ("tensile", "holes3k", "plate100k")}


def variants_for(prob, V):
    from variants_util import make_variants
    xy, mat, u, f = make_variants(prob, V, seed=11)
    u[1:2], f[1:2] = u[0:1], f[0:1]  # (no 1e-3 x variant here: every variant runs about as long as a single solve)
    return xy, mat, u, f


def leg_sequential(names_V):
    from magnetite_amd import Context
    from variants_util import variant_problem
    out, probs = {}, problems()
    for name, V in names_V.items():
        prob = probs[name]
        xy, mat, u, f = variants_for(prob, V)
        vps = [variant_problem(prob, xy[i], mat[i], u[i], f[i]) for i in range(V)]
        with Context(device=0) as c:
            c.solve(vps[0])  # warm-up
            walls = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                for vp in vps:
                    c.upload_problem(vp)
                    c.run()
                    c.download()
                walls.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"wall": med(walls)}
    return out


def leg_variants(names_V):
    from magnetite_amd import Context
    out, probs = {}, problems()
    for name, V in names_V.items():
        prob = probs[name]
        xy, mat, u, f = variants_for(prob, V)
        with Context(device=0) as c:
            c.upload_problem(prob)
            c.set_variants(xy, mat, u, f)
            c.run_variants()  # warm-up
            walls, phases = [], {k: [] for k in ("permute", "assemble", "rhs_and_blocks", "cg_launches", "post")}
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                c.run_variants()
                for i in range(V):
                    c.download_variant(i)
                walls.append((time.perf_counter() - t0) * 1e3)
                info = c.variants_info()
                sts = [c.variant_stats(i) for i in range(V)]
                step = max(1, info["variants_per_launch"])
                phases["permute"].append(sts[0]["ms_element"])
                phases["assemble"].append(sts[0]["ms_assemble"])
                phases["rhs_and_blocks"].append(sts[0]["ms_bc"])
                phases["cg_launches"].append(sum(s["ms_cg"] for s in (sts[::step] if info["variants_per_launch"] else sts)))
                phases["post"].append(sts[0]["ms_post"])
        out[name] = {"info": info, "wall": med(walls), "phases": {k: med(v) for k, v in phases.items()}}
    return out


def shapes():
    from magnetite_amd import Context
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, check=True)
    cus = int(r.stdout.split()[-1])
    with Context(device=0) as c:
        st = c.solve(problems()["holes3k"])
    G = -(-st["num_tiles"] // max(1, st["tiles_per_workgroup"]))
    return cus, {"tensile": 256, "holes3k": max(1, cus // G) + 3, "plate100k": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants.json"))
    ap.add_argument("--leg", choices=("sequential",), help=argparse.SUPPRESS)
    ap.add_argument("--shapes", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == "sequential":  # child process: the package of MAG_PROBE_PACKAGE_ROOT
        print("RESULT " + json.dumps(leg_sequential(json.loads(a.shapes))), flush=True)
        return
    cus, names_V = shapes()
    env = dict(os.environ)
    if a.baseline_tree:
        env["MAG_PROBE_PACKAGE_ROOT"] = os.path.abspath(a.baseline_tree)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "sequential", "--shapes", json.dumps(names_V)], env=env,
                       capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit("sequential leg failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    seq = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    var = leg_variants(names_V)
    rows = []
    for name, V in names_V.items():
        rows.append({"mesh": name, "variants": V, "run_variants": var[name], "sequential": seq[name],
                     "speedup": round(seq[name]["wall"]["median_ms"] / var[name]["wall"]["median_ms"], 3)})
        print(json.dumps(rows[-1]), flush=True)
    doc = {"compute_units": cus, "baseline_library": "the parent commit's build" if a.baseline_tree else "this build",
           "repeats": REPEATS, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
