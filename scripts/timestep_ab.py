"""A/B of builds of the library over the time-stepping passes (mag_run_transient, mag_run_explicit with either kinematics,
mag_run_transient_tl) and mag_run_newton in ONE GPU session: the same bits, and the same speed as far as the session can tell.  Every library is loaded by a child process
of its own through MAG_LIB_PATH; the libraries alternate over the rounds.  The first library named is the parent, the others are
compared with it.

Bits (--rounds-bits, default 2): on holes3k and two_fans, with the tile-local tables and under op_variant=1, the implicit pass at
cg = 0 and cg = 4, the linear and the total-Lagrangian explicit pass; every run records three probes, the energies, a snapshot
every 5 steps and (explicit) a row every 3, and is a 40-step run followed by a resumed 24-step run.  A sha256 of every array of
download_transient() and the info words are printed; every library must agree with the parent on each.  Likewise mag_run_newton
(2 increments, line search off and on, cg = 0 and 4: every array of download_newton()), mag_run_transient_tl (a 10-step run and a
resumed 6-step run, cg = 0 and 4: download_transient() and download_transient_tl()) and the three single evaluations
(mag_assemble_tangent, mag_assemble_effective_tangent, mag_internal_force) at a non-zero state.

Speed (--rounds, default 7): on plate100k, 4096 explicit steps without records at 0.9 dt_bound for both kinematics and 256
implicit steps at dt = T1 / 200, cg = 0 (T1 from the host's eigensolver, tests/modal_ref.py); on the same plate as the cantilever of
profiles/newton.json and profiles/transient_tl.json, the first of the eight increments of mag_run_newton and 8 steps of
mag_run_transient_tl at that profile's dt.  A child does one run of each to
warm up and one timed run of each (the passes synchronise before they return); a figure is the median over the rounds.  The
control is the parent library once more under another file name: twice the relative difference between the two parent legs is
what the session cannot resolve, and a library passes a figure when its median exceeds the parent's by no more than that.
    python scripts/timestep_ab.py [--out profiles/timestep_refactor.json] parent.so new.so ..."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RHO = 2700.0
PROBES = (1, 100, 401)
EX_STEPS, IM_STEPS = 4096, 256
TL_STEPS, TOTAL_LOAD = 8, 3e8
FIGURES = ("explicit_linear_4096_steps", "explicit_tl_4096_steps", "implicit_cg0_256_steps", "newton_cantilever_1_increment",
           "transient_tl_cantilever_8_steps")


def meshes():
    from magnetite_amd import meshgen
    xy, tri, cx, cy = meshgen._grid(64, 64, 1.0, 1.0)  # plate(64) minus two cells that leave node (21, 21) with two fans
    keep = np.ones(cx.shape[0], dtype=bool)
    keep[[20 * 64 + 20, 21 * 64 + 21]] = False
    return {"holes3k": meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3)),
            "two_fans": meshgen.config_fixed_left_point_load(meshgen._compact(xy, tri, keep, "pinched_plate"))}


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def cantilever():
    """the plate of plate100k clamped on the left, its right edge pulled down by TOTAL_LOAD (scripts/newton_probe.py)"""
    from magnetite_amd import meshgen
    mesh = meshgen.plate(224)
    prob = meshgen.config_fixed_left_point_load(mesh, load=0.0)
    right = np.flatnonzero(mesh.xy[:, 0] > mesh.xy[:, 0].max() - 1e-9)
    prob.f_in[:] = 0.0
    prob.f_in[2 * right + 1] = -TOTAL_LOAD / len(right)
    return prob


def bits_leg():
    """child process: every digest and info word of the library MAG_LIB_PATH names; one JSON line"""
    from magnetite_amd import Context
    out = {}
    for mesh, prob in meshes().items():
        for cname, ckw in (("tables", {}), ("op_variant1", dict(op_variant=1))):
            with Context(device=0, **ckw) as c:
                c.upload_problem(prob)
                dt_im = 40.0 * c.explicit_dt(RHO)["dt_bound"]
                rec = dict(probes=PROBES, energies=True, snapshot_every=5, density=RHO)
                passes = {"implicit_cg0": lambda **kw: c.run_transient(dt=dt_im, cg=0, rayleigh=(5.0, 1e-7), **rec, **kw),
                          "implicit_cg4": lambda **kw: c.run_transient(dt=dt_im, cg=4, rayleigh=(5.0, 1e-7), **rec, **kw),
                          "explicit_linear": lambda **kw: c.run_explicit(record_every=3, rayleigh=(5.0, 1e-8), **rec, **kw),
                          "explicit_tl": lambda **kw: c.run_explicit(record_every=3, rayleigh=(5.0, 0.0), kinematics="tl", **rec, **kw)}
                for pname, run in passes.items():
                    for part, steps, resume in (("first", 40, False), ("resumed", 24, True)):
                        run(steps=steps, resume=resume, amplitude=1.0 + 0.5 * np.sin(0.3 * np.arange(steps + 1)))
                        got = c.download_transient()
                        key = f"{mesh}/{cname}/{pname}/{part}"
                        for k in sorted(got):
                            out[f"{key}/{k}"] = digest(np.asarray(got[k]))
                        out[f"{key}/info"] = list(c.transient_info().values())
                for cg in (0, 4):
                    for search in (0, 3):
                        c.run_newton(increments=2, line_search=search, cg=cg, probes=PROBES, snapshots=True)
                        got, key = c.download_newton(), f"{mesh}/{cname}/newton_cg{cg}_search{search}"
                        for k in sorted(got):
                            out[f"{key}/{k}"] = digest(np.asarray(got[k]))
                        out[f"{key}/info"] = list(c.newton_info().values())
                    for part, steps, resume in (("first", 10, False), ("resumed", 6, True)):
                        c.run_transient_tl(steps=steps, dt=dt_im, cg=cg, rayleigh=(5.0, 0.0), resume=resume,
                                           amplitude=1.0 + 0.5 * np.sin(0.3 * np.arange(steps + 1)), **rec)
                        got, key = dict(c.download_transient(), **c.download_transient_tl()), f"{mesh}/{cname}/transient_tl_cg{cg}/{part}"
                        for k in sorted(got):
                            out[f"{key}/{k}"] = digest(np.asarray(got[k]))
                        out[f"{key}/info"] = list(c.transient_info().values()) + list(c.transient_tl_info().values())
                u = 2e-4 * np.sin(np.arange(2.0 * c.N))
                f, W, inverted = c.internal_force(u)
                evaluations = dict(tangent=c.assemble_tangent(u), effective_tangent=c.assemble_effective_tangent(u, 0.25 * dt_im ** 2, 1.01, RHO),
                                   internal_force=f, W=np.float64(W), inverted=np.int32(inverted))
                for k, v in evaluations.items():
                    out[f"{mesh}/{cname}/evaluations/{k}"] = digest(np.asarray(v))
    print(json.dumps(out))


def speed_leg(dt_im):
    """child process: one warm-up and one timed run of every figure; one JSON line of wall ms"""
    from magnetite_amd import Context, meshgen
    prob = meshgen.baseline_problem("plate100k")
    with Context(device=0) as c:
        c.upload_problem(prob)
        dt = 0.9 * c.explicit_dt(RHO)["dt_bound"]
        runs = {"explicit_linear_4096_steps": lambda: c.run_explicit(EX_STEPS, dt=dt, density=RHO),
                "explicit_tl_4096_steps": lambda: c.run_explicit(EX_STEPS, dt=dt, density=RHO, kinematics="tl"),
                "implicit_cg0_256_steps": lambda: c.run_transient(IM_STEPS, dt_im, density=RHO, cg=0)}
        wall = {}
        for name, run in runs.items():
            run()
            t0 = time.perf_counter()
            run()
            wall[name] = 1e3 * (time.perf_counter() - t0)
            wall[name + "/launches_or_iterations"] = c.transient_info()["cg_iterations"]
    # the cantilever's figures, each on a context of its own: where the buffers of a pass lie then does not depend on the passes
    # that ran before it
    with open(os.path.join(ROOT, "profiles", "transient_tl.json")) as fh:
        dt_tl = json.load(fh)["dt"]
    prob = cantilever()
    for name, run, count in (
            ("newton_cantilever_1_increment", lambda c: c.run_newton(increments=1, load_factors=[0.125], cg=0),
             lambda c: c.newton_info()["cg_iterations_total"]),
            ("transient_tl_cantilever_8_steps", lambda c: c.run_transient_tl(TL_STEPS, dt_tl, density=RHO, lumped=True, newton_tol=1e-10, cg_tol=1e-10),
             lambda c: c.transient_tl_info()["cg_iterations_total"])):
        with Context(device=0) as c:
            c.upload_problem(prob)
            run(c)
            t0 = time.perf_counter()
            run(c)
            wall[name] = 1e3 * (time.perf_counter() - t0)
            wall[name + "/launches_or_iterations"] = count(c)
    print(json.dumps(wall))


def child(lib, *args):
    env = dict(os.environ, MAG_LIB_PATH=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"{lib} {args}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timestep_refactor.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rounds-bits", type=int, default=2)
    ap.add_argument("--bits-leg", action="store_true")
    ap.add_argument("--speed-leg", type=float, default=None)
    ap.add_argument("libs", nargs="*")
    a = ap.parse_args()
    if a.bits_leg:
        return bits_leg()
    if a.speed_leg is not None:
        return speed_leg(a.speed_leg)
    if len(a.libs) < 2:
        ap.error("name the parent's library and at least one other")
    parent, others = a.libs[0], a.libs[1:]

    # ---- the bits
    bits, agree = {}, True
    for rnd in range(a.rounds_bits):
        for lib in a.libs:
            got = child(lib, "--bits-leg")
            for k in sorted(got):
                print(rnd, os.path.basename(os.path.dirname(os.path.abspath(lib))), os.path.basename(lib), k, got[k], flush=True)
            differ = [k for k in got if bits.setdefault(parent, got).get(k) != got[k]] + [k for k in bits[parent] if k not in got]
            if differ:
                agree = False
                print("DIFFERS from the parent's first leg:", lib, differ[:20], flush=True)
    print(json.dumps({"digests_and_info_words": len(bits[parent]), "all_agree": agree}), flush=True)

    # ---- the speed: parent, the others, the control (the parent's file under another name), alternated
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import modal_ref
    from magnetite_amd import meshgen
    K, M, free = modal_ref.matrices(meshgen.baseline_problem("plate100k"), RHO)
    lam, _ = modal_ref.eigenpairs(K, M, free, 2)
    T1 = 2.0 * np.pi / float(np.sqrt(lam[0]))
    with tempfile.TemporaryDirectory() as tmp:
        control = os.path.join(tmp, "libmagnetite_hip_control.so")
        shutil.copyfile(parent, control)
        legs = {"parent": parent, **{f"new{'' if len(others) == 1 else k}": lib for k, lib in enumerate(others)}, "control": control}
        wall = {leg: {f: [] for f in FIGURES} for leg in legs}
        counts = {}
        for rnd in range(a.rounds):
            for leg, lib in legs.items():
                got = child(lib, "--speed-leg", repr(T1 / 200.0))
                for f in FIGURES:
                    wall[leg][f].append(got[f])
                    counts.setdefault(f, set()).add(got[f + "/launches_or_iterations"])
                print(rnd, leg, {f: round(got[f], 3) for f in FIGURES}, flush=True)

    out = {"mesh": "plate100k", "rounds": a.rounds, "T1": T1, "implicit_dt": T1 / 200.0, "libraries": {k: os.path.basename(v) for k, v in legs.items()},
           "bits": {"meshes": ["holes3k", "two_fans"], "rounds": a.rounds_bits, "digests_and_info_words": len(bits[parent]), "all_agree": agree},
           "figures": {}}
    for f in FIGURES:
        med = {leg: statistics.median(wall[leg][f]) for leg in legs}
        control_diff = abs(med["control"] - med["parent"]) / med["parent"]
        margin = 2.0 * control_diff
        out["figures"][f] = {"wall_ms": {leg: {"median": round(med[leg], 4), "all": [round(x, 4) for x in wall[leg][f]]} for leg in legs},
                             "launches_or_iterations": sorted(counts[f]), "control_relative_difference": control_diff, "margin": margin,
                             "verdicts": {leg: {"over_parent": med[leg] / med["parent"] - 1.0, "within_margin": bool(med[leg] <= med["parent"] * (1.0 + margin))}
                                          for leg in legs if leg not in ("parent", "control")}}
    print(json.dumps(out, indent=1))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    ok = agree and all(v["within_margin"] for f in out["figures"].values() for v in f["verdicts"].values())
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
