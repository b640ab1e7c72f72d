"""mag_run_explicit with kinematics = MAG_KIN_TOTAL_LAGRANGIAN on the 100k-triangle plate under the cantilever load applied at
t = 0: what the total-Lagrangian step costs next to the linear one.  4096 steps without records, median of 7, the legs
alternated in one session, all at the same dt = 0.9 dt_bound.

Legs:
  (a) the total-Lagrangian step of this build (one launch of k_explicit_tl_step a step: no matrix is read);
  (b) the linear step of this build (k_explicit_step over K's tile-local block rows);
  (c) the linear step of the PARENT commit's library (--parent-lib, loaded by a child process through MAG_LIB_PATH; its struct has
      `reserved` where this build has `kinematics`: 0 either way); without --parent-lib this build's library runs that leg and the
      file says so.
Written down with them: the compulsory bytes of either step and the time they would take at the HBM and Infinity-Cache rates
DESIGN.md (EX) quotes; the kernels' own times where a rocprofv3 --kernel-trace --stats file of a run of its own is given
(--kernel-stats), the gap between wall time per step and kernel time, and what bounds the kernel.
    python scripts/explicit_tl_probe.py [--parent-lib PATH] [--kernel-stats kernel_stats.csv] [--out profiles/explicit_tl.json]
    python scripts/explicit_tl_probe.py --trace-run    (the short run to put under rocprofv3: 512 steps of either kinematics)"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS, STEPS, RHO = 7, 4096, 2700.0
HBM_TBS, L3_TBS = 6.3, 8.6  # achievable HBM3E stream; uniformly gathered rows out of the Infinity Cache (EX)


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def linear_leg(a):
    """child process: the linear step of whatever library MAG_LIB_PATH names, STEPS steps of --dt, REPEATS times; one JSON line"""
    from magnetite_amd import Context, meshgen
    prob = meshgen.baseline_problem(a.mesh)
    wall = []
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.run_explicit(8, dt=a.dt, density=RHO)
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            c.run_explicit(STEPS, dt=a.dt, density=RHO)
            wall.append(1e3 * (time.perf_counter() - t0))
        u = c.download_transient()["u"]
    print(json.dumps({"wall_ms": wall, "u_norm": float(np.linalg.norm(u))}))


def kernel_times_us(path):
    """the averages of k_explicit_tl_step and k_explicit_step in a rocprofv3 --kernel-trace --stats file (ns columns)"""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            key = "k_explicit_tl_step" if "k_explicit_tl_step" in name else ("k_explicit_step" if "k_explicit_step" in name else None)
            if key:
                avg = row.get("AverageNs") or row.get("Average")
                out[key] = {"calls": int(row.get("Calls", 0)), "average_us": round(float(avg) / 1e3, 4),
                            "min_us": round(float(row.get("MinNs", "nan")) / 1e3, 4), "max_us": round(float(row.get("MaxNs", "nan")) / 1e3, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explicit_tl.json"))
    ap.add_argument("--mesh", default="plate100k")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--linear-leg", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--dt", type=float, default=0.0)
    a = ap.parse_args()
    if a.linear_leg:
        return linear_leg(a)
    from magnetite_amd import Context, meshgen
    prob = meshgen.baseline_problem(a.mesh)
    N, E = prob.mesh.num_nodes, prob.mesh.num_elements
    if a.trace_run:
        with Context(device=0) as c:
            c.upload_problem(prob)
            c.run_explicit(512, density=RHO, kinematics="tl")
            c.run_explicit(512, density=RHO)
        return

    with Context(device=0) as c:
        c.upload_problem(prob)
        bound = c.explicit_dt(RHO)
        dt = 0.9 * bound["dt_bound"]
        blocks = c.assemble_csr()[2].size // 4
        c.run()  # (a static solve: mag_get_stats then holds the sizes of the tile-local tables)
        stats = c.stats()
        legs ={"total_lagrangian": dict(kinematics="tl"), "linear": dict()}
        wall = {k: [] for k in legs}
        info, u = {}, {}
        for kw in legs.values():  # (order, pattern, K, the table, the buffers)
            c.run_explicit(8, dt=dt, density=RHO, **kw)
        for rep in range(REPEATS):
            for name, kw in legs.items():
                t0 = time.perf_counter()
                c.run_explicit(STEPS, dt=dt, density=RHO, **kw)
                wall[name].append(1e3 * (time.perf_counter() - t0))
                info[name] = c.transient_info()
                u[name] = c.download_transient()["u"]
    for name in legs:  # the structural condition: a step without records is one launch (words 2 and 3)
        assert (info[name]["preconditioner"], info[name]["cg_iterations"]) == (1, STEPS + 1), info[name]
    assert info["total_lagrangian"]["cg_kernel"] == 7 and info["linear"]["cg_kernel"] == 6

    env = dict(os.environ)
    if a.parent_lib:
        env["MAG_LIB_PATH"] = os.path.abspath(a.parent_lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--linear-leg", "--mesh", a.mesh, "--dt", repr(dt)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    parent = json.loads(r.stdout.strip().splitlines()[-1])

    ring_words = int(stats["ell_entries"])  # 4-byte words of the tile-local ring table, read once a step
    halo = int(stats["halo_nodes"])
    # records in and out, coordinates, u_in, load, mass, mask per node; the ring words; a halo node's record, mask, u_in, coordinates
    tl_bytes = N * (48 + 48 + 16 + 16 + 16 + 8 + 1) + 4 * ring_words + halo * (48 + 1 + 16 + 16 + 4)
    lin_bytes = blocks * (32 + 2) + N * (48 + 48 + 16 + 16 + 8 + 1)
    us_step = {k: 1e3 * statistics.median(v) / STEPS for k, v in wall.items()}
    parent_us = 1e3 * statistics.median(parent["wall_ms"]) / STEPS

    def roofs(nbytes):
        return {"total": nbytes, "per_node": round(nbytes / N, 1), "us_at_hbm_%.1f_TBs" % HBM_TBS: round(nbytes / HBM_TBS / 1e6, 4),
                "us_at_infinity_cache_%.1f_TBs" % L3_TBS: round(nbytes / L3_TBS / 1e6, 4)}

    out = {"mesh": a.mesh, "nodes": N, "elements": E, "blocks_of_K": blocks, "ring_words": ring_words, "halo_nodes": halo,
           "tile_nodes": 512, "tiles": int(stats["num_tiles"]), "dt_bound": bound["dt_bound"], "dt": dt, "steps": STEPS, "repeats": REPEATS,
           "step": {k: {"wall_ms": summary(wall[k]), "us_per_step": round(us_step[k], 4)} for k in us_step},
           "parent_linear": {"library": "parent commit (MAG_LIB_PATH)" if a.parent_lib else "this build (no --parent-lib given)",
                             "wall_ms": summary(parent["wall_ms"]), "us_per_step": round(parent_us, 4),
                             "final_u_norm_against_this_builds_linear": abs(parent["u_norm"] - float(np.linalg.norm(u["linear"]))) /
                             float(np.linalg.norm(u["linear"]))},
           "total_lagrangian_over_linear": round(us_step["total_lagrangian"] / us_step["linear"], 3),
           "linear_over_parent_linear": round(us_step["linear"] / parent_us, 3),
           "final_u_tl_against_linear": float(np.linalg.norm(u["total_lagrangian"] - u["linear"]) / np.linalg.norm(u["linear"])),
           "compulsory_bytes_per_step": {"total_lagrangian": roofs(tl_bytes), "linear": roofs(lin_bytes)}}
    if a.kernel_stats:
        k = kernel_times_us(a.kernel_stats)
        out["kernel"] = k
        for key, nbytes, leg in (("k_explicit_tl_step", tl_bytes, "total_lagrangian"), ("k_explicit_step", lin_bytes, "linear")):
            if key in k:
                k[key]["wall_minus_kernel_us_per_step"] = round(us_step[leg] - k[key]["average_us"], 4)
                k[key]["share_of_hbm_roof"] = round(nbytes / HBM_TBS / 1e6 / k[key]["average_us"], 4)
                k[key]["share_of_infinity_cache_roof"] = round(nbytes / L3_TBS / 1e6 / k[key]["average_us"], 4)
    else:
        out["kernel"] = "not measured (no --kernel-stats given)"
    print(json.dumps(out, indent=1))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
