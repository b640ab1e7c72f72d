"""A/B of builds of the library over the three time-stepping passes (mag_run_transient, mag_run_explicit with either kinematics)
in ONE GPU session: the same bits, and the same speed as far as the session can tell.  Every library is loaded by a child process
of its own through MAG_LIB_PATH; the libraries alternate over the rounds.  The first library named is the parent, the others are
compared with it.

Bits (--rounds-bits, default 2): on holes3k and two_fans, with the tile-local tables and under op_variant=1, the implicit pass at
cg = 0 and cg = 4, the linear and the total-Lagrangian explicit pass; every run records three probes, the energies, a snapshot
every 5 steps and (explicit) a row every 3, and is a 40-step run followed by a resumed 24-step run.  A sha256 of every array of
download_transient() and the info words are printed; every library must agree with the parent on each.

Speed (--rounds, default 7): on plate100k, 4096 explicit steps without records at 0.9 dt_bound for both kinematics and 256
implicit steps at dt = T1 / 200, cg = 0 (T1 from the host's eigensolver, tests/modal_ref.py).  A child does one run of each to
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
FIGURES = ("explicit_linear_4096_steps", "explicit_tl_4096_steps", "implicit_cg0_256_steps")


def meshes():
    from magnetite_amd import meshgen
    xy, tri, cx, cy = meshgen._grid(64, 64, 1.0, 1.0)  # plate(64) minus two cells that leave node (21, 21) with two fans
    keep = np.ones(cx.shape[0], dtype=bool)
    keep[[20 * 64 + 20, 21 * 64 + 21]] = False
    return {"holes3k": meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(56), 3)),
            "two_fans": meshgen.config_fixed_left_point_load(meshgen._compact(xy, tri, keep, "pinched_plate"))}


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


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
        for name in FIGURES:
            runs[name]()
            t0 = time.perf_counter()
            runs[name]()
            wall[name] = 1e3 * (time.perf_counter() - t0)
            wall[name + "/launches_or_iterations"] = c.transient_info()["cg_iterations"]
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
