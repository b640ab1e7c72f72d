"""Writes profiles/roundoff_parity.json: the figures behind the bars of tests/test_roundoff_parity_gpu.py.

  python scripts/roundoff_parity.py [OUT.json]

Runs that test file once with MAG_ROUNDOFF_RECORD set (per workload, cg_variant and stop rule: GPU and oracle iterations,
GPU and oracle true residuals, rel-L2 to the direct solve, the worst reaction ratio to its round-off bar, stress
mismatches and excluded elements), then the six sampled cases of tests/test_fullsize_parity_gpu.py for their iteration
counts, and sums up the largest |gpu - oracle| iteration difference per workload, which the iteration bars of both test
files are twice of.  Nothing more is started on the GPU if the test run ended by a signal or a time limit.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "roundoff_parity.json")
SAMPLED = [("hole1m", 2), ("hole1m", 1), ("plate4m", 1), ("multihole16m", 1), ("frontal1m", 2), ("frontal1m", 1)]

with tempfile.TemporaryDirectory() as tmp:
    rec = os.path.join(tmp, "record.json")
    rc = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_roundoff_parity_gpu.py"), "-m", "gpu",
                         "-q", "-s", "-p", "no:cacheprovider"], env=dict(os.environ, MAG_ROUNDOFF_RECORD=rec), cwd=ROOT,
                        timeout=900).returncode
    if rc not in (0, 1):
        raise SystemExit(f"the test run ended with status {rc}: nothing more is run")
    cases = json.load(open(rec))

from magnetite_amd import Context, _lib, meshgen  # noqa: E402

for name, variant in SAMPLED:
    fx = np.load(os.path.join(ROOT, "tests", "golden", f"fullsize_{name}.npz"), allow_pickle=False)
    with Context(device=0, stop_mode=_lib.MAG_STOP_REL, tol=float(fx["rel_tol"]), cg_variant=variant) as c:
        out = c.solve(meshgen.baseline_problem(name))
    cases[f"{name} cg_variant={variant} rel {float(fx['rel_tol']):g} (sampled full-size case)"] = dict(
        gpu_iterations=int(out["iterations"]), oracle_iterations=int(fx["iterations"]), oracle_solver=str(fx["solver"]))
    print(name, variant, int(out["iterations"]), int(fx["iterations"]), flush=True)

largest = {}
for key, c in cases.items():
    if "oracle_iterations" in c:
        w = key.split()[0]
        largest[w] = max(largest.get(w, 0), abs(c["gpu_iterations"] - c["oracle_iterations"]))
json.dump(dict(test_run_status=rc, largest_iteration_difference=largest, cases=cases), open(OUT, "w"), indent=1, sort_keys=True)
print(json.dumps(largest), "->", OUT)
