"""mag_run_explicit on the 100k-triangle plate under the cantilever load applied at t = 0: what a central-difference step costs
when it is one fused launch.  Median of 7, the legs alternated in one session.

Legs:
  (a) 4096 explicit steps at 0.9 dt_bound, without records and with record_every = 64 (three probes and the energies): ms, us per step;
  (b) the baseline: the PARENT commit's library (--parent-lib, loaded by a child process through MAG_LIB_PATH) running the same
      arithmetic -- transient(beta=0, gamma=0.5, lumped=True, cg=1), a CG solve on a diagonal matrix per step -- at the same dt for
      256 steps; without --parent-lib this build's library runs that leg and the file says so;
  (c) for context, the same physical time span by the implicit pass at dt = T1 / 200 (cg = 0, average acceleration).
Written down with them: the compulsory bytes of a step (the block rows' values and slots once, the state records in and out,
masses, loads, supports) and the time they would take at the HBM and Infinity-Cache rates of the microarchitecture guide; the
kernel's own time where a rocprofv3 --kernel-trace --stats file of a run of its own is given (--kernel-stats), and so the gap
between wall time per step and kernel time; whether the host's enqueue or the kernel bounds a step.
    python scripts/explicit_probe.py [--parent-lib PATH] [--kernel-stats kernel_stats.csv] [--out profiles/explicit.json]
    python scripts/explicit_probe.py --trace-run      (the short run to put under rocprofv3: 512 steps, no records)"""
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
sys.path.insert(1, os.path.join(ROOT, "tests"))
REPEATS, STEPS, BASE_STEPS, RHO = 7, 4096, 256, 2700.0
HBM_TBS, L3_TBS = 6.3, 8.6  # achievable HBM3E stream; uniformly gathered rows out of the Infinity Cache (the guide's tables)


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def baseline_leg(a):
    """child process: the implicit pass at beta = 0 on the lumped mass, 256 steps of --dt, REPEATS times; one JSON line"""
    from magnetite_amd import Context, meshgen
    prob = meshgen.baseline_problem(a.mesh)
    wall = []
    with Context(device=0) as c:
        c.upload_problem(prob)
        kw = dict(beta=0.0, gamma=0.5, lumped=True, cg=1)
        c.run_transient(4, a.dt, RHO, **kw)
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            c.run_transient(BASE_STEPS, a.dt, RHO, **kw)
            wall.append(1e3 * (time.perf_counter() - t0))
        info = c.transient_info()
        u = c.download_transient()["u"]
    print(json.dumps({"wall_ms": wall, "cg_iterations": info["cg_iterations"], "u_norm": float(np.linalg.norm(u)),
                      "u_head": [float(x) for x in u[:8]]}))


def kernel_time_us(path):
    """the average of k_explicit_step in a rocprofv3 --kernel-trace --stats file (ns columns)"""
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            if "k_explicit_step" in name:
                avg = row.get("AverageNs") or row.get("Average")
                return {"calls": int(row.get("Calls", 0)), "average_us": round(float(avg) / 1e3, 4),
                        "min_us": round(float(row.get("MinNs", "nan")) / 1e3, 4), "max_us": round(float(row.get("MaxNs", "nan")) / 1e3, 4)}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explicit.json"))
    ap.add_argument("--mesh", default="plate100k")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--baseline-leg", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--dt", type=float, default=0.0)
    a = ap.parse_args()
    if a.baseline_leg:
        return baseline_leg(a)
    from magnetite_amd import Context, meshgen
    prob = meshgen.baseline_problem(a.mesh)
    N = prob.mesh.num_nodes
    if a.trace_run:
        with Context(device=0) as c:
            c.upload_problem(prob)
            c.run_explicit(512, density=RHO)
        return
    import modal_ref
    K, M, free = modal_ref.matrices(prob, RHO, True)
    lam, _ = modal_ref.eigenpairs(K, M, free, 2)
    T1 = 2.0 * np.pi / float(np.sqrt(lam[0]))
    probes = [1, N, 2 * N - 1]

    with Context(device=0) as c:
        c.upload_problem(prob)
        bound = c.explicit_dt(RHO)
        dt = 0.9 * bound["dt_bound"]
        blocks = c.assemble_csr()[2].size // 4
        legs = {"no records": dict(), "record_every 64": dict(record_every=64, probes=probes, energies=True)}
        span = STEPS * dt
        im_steps = max(1, int(np.ceil(span / (T1 / 200.0))))
        wall = {k: [] for k in legs}
        wall["implicit"] = []
        for kw in legs.values():  # (order, pattern, K, the table, the buffers)
            c.run_explicit(8, density=RHO, **kw)
        c.run_transient(2, span / im_steps, RHO)
        info = {}
        for rep in range(REPEATS):
            for name, kw in legs.items():
                t0 = time.perf_counter()
                c.run_explicit(STEPS, density=RHO, **kw)
                wall[name].append(1e3 * (time.perf_counter() - t0))
                info[name] = c.transient_info()
                if name == "no records":
                    u_ex = c.download_transient()["u"]
            t0 = time.perf_counter()
            c.run_transient(im_steps, span / im_steps, RHO)
            wall["implicit"].append(1e3 * (time.perf_counter() - t0))
            info["implicit"] = c.transient_info()
        # the same arithmetic by this build's implicit pass, for the check of leg (b)'s result
        c.run_explicit(BASE_STEPS, density=RHO)
        u_256 = c.download_transient()["u"]
        fused, launches = info["no records"]["preconditioner"], info["no records"]["cg_iterations"]  # (words 2 and 3)
    assert launches == STEPS + 1, launches  # the structural condition: a step without records is one launch

    env = dict(os.environ)
    if a.parent_lib:
        env["MAG_LIB_PATH"] = os.path.abspath(a.parent_lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-leg", "--mesh", a.mesh, "--dt", repr(dt)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    base = json.loads(r.stdout.strip().splitlines()[-1])

    entries_bytes = blocks * (32 + 2)
    node_bytes = N * (48 + 48 + 16 + 16 + 8 + 1)
    compulsory = entries_bytes + node_bytes
    us_step = {k: 1e3 * statistics.median(v) / STEPS for k, v in wall.items() if k != "implicit"}
    base_us = 1e3 * statistics.median(base["wall_ms"]) / BASE_STEPS
    out = {"mesh": a.mesh, "nodes": N, "elements": prob.mesh.num_elements, "blocks_of_K": blocks, "T1": T1, "dt_bound": bound["dt_bound"],
           "dt": dt, "T1_over_dt": T1 / dt, "steps": STEPS, "repeats": REPEATS, "fused": fused, "step_launches": launches,
           "explicit": {k: {"wall_ms": summary(wall[k]), "us_per_step": round(us_step[k], 4)} for k in us_step},
           "baseline_parent_implicit_beta0": {
               "library": "parent commit (MAG_LIB_PATH)" if a.parent_lib else "this build (no --parent-lib given)", "steps": BASE_STEPS,
               "wall_ms": summary(base["wall_ms"]), "us_per_step": round(base_us, 4), "cg_iterations": base["cg_iterations"],
               "final_u_norm_against_explicit_256": abs(base["u_norm"] - float(np.linalg.norm(u_256))) / float(np.linalg.norm(u_256)),
               "over_explicit_no_records": round(base_us / us_step["no records"], 2)},
           "implicit_same_span": {"steps": im_steps, "dt": span / im_steps, "wall_ms": summary(wall["implicit"]),
                                  "cg_iterations": info["implicit"]["cg_iterations"],
                                  "over_explicit_no_records": round(statistics.median(wall["implicit"]) / statistics.median(wall["no records"]), 3)},
           "compulsory_bytes_per_step": {"block_rows": entries_bytes, "state_masses_loads_supports": node_bytes, "total": compulsory,
                                         "us_at_hbm_%.1f_TBs" % HBM_TBS: round(compulsory / HBM_TBS / 1e6, 4),
                                         "us_at_infinity_cache_%.1f_TBs" % L3_TBS: round(compulsory / L3_TBS / 1e6, 4),
                                         "working_set_MB": round((entries_bytes + 2 * 48 * N + N * 41) / 1e6, 2)}}
    if a.kernel_stats:
        k = kernel_time_us(a.kernel_stats)
        out["kernel"] = k
        if k:
            gap = us_step["no records"] - k["average_us"]
            out["kernel"]["wall_minus_kernel_us_per_step"] = round(gap, 4)
            out["kernel"]["share_of_hbm_roof"] = round(compulsory / HBM_TBS / 1e6 / k["average_us"], 4)
            out["kernel"]["share_of_infinity_cache_roof"] = round(compulsory / L3_TBS / 1e6 / k["average_us"], 4)
            out["kernel"]["bound_by"] = ("the host's enqueue and the kernel boundary (a captured graph of the steps is the named follow-up)"
                                         if gap > k["average_us"] else "the kernel")
    else:
        out["kernel"] = "not measured (no --kernel-stats given)"
    print(json.dumps(out, indent=1))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
