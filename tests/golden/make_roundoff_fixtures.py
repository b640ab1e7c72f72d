"""Generates tests/golden/roundoff_<workload>.npz: a BASELINE-size workload solved to round-off, three ways, SAMPLED.

  python tests/golden/make_roundoff_fixtures.py hole1m frontal1m

tests/golden/fullsize_*.npz hold the oracle's CG stopped where bench.py stops it (relative residual 1e-8), which on
hole1m is 6e-7 away from the discrete solution.  These files hold, of the oracle's own K_ff x = b (assemble_sparse +
reduce_system, the matrix the existing bit-for-bit test pins the library's assembly to):

  direct     scipy.sparse.linalg.splu (MMD_AT_PLUS_A, SymmetricMode, diag_pivot_thresh=0) followed by iterative
             refinement until the step stops shrinking.  NOT a CG: the arbiter.  Its own error bar -- the relative true
             residual and the relative size of the last refinement step -- is recorded with it.
  rnorm      oracle.cg under STOP_RNORM at TARGET_CG_COST, the reference's stop rule (solver.rs:18-19,153-154) and the
             library's default, then reactions and stress as orc_run_sparse forms them.
  rnorm_sq   the same under STOP_RNORM_SQ (the other reading of argmin's cost).

per CG rule: iterations, final (recurred) cost, the TRUE residual |b - K_ff x| (relative and absolute), the rel-L2
distance to the direct solution over all free DOFs, norms, and u / f / stress at the positions make_fullsize_fixtures.py
samples (same sample_indices, same seed); for the direct solution the same sampled u, f (oracle K.spmv) and stress
(oracle.stress).  The mesh checksums are those of the fullsize fixtures.

The three solves of a workload run as separate processes (`--part`, one thread each for the CG and for SuperLU; the
assembly uses 8) and exchange whole vectors through a temporary folder; the parent samples them.  Deterministic: the
serial CG and SuperLU have a fixed order of operations, the OpenMP assembly gives the serial one's bits.
Ran here on 8 cores, both workloads and all six solves side by side, in 7 minutes wall (22 CPU-minutes): the rnorm CG is
the longest of each workload (hole1m 204 s, frontal1m 414 s), the factorisation needs 29 s (hole1m) / 113 s (frontal1m)
and about 6.4 GB at its peak.  Run times are printed, not stored: two runs give the same arrays.

PARITY UNPINNED: as for make_fullsize_fixtures.py, the reference cannot run these sizes and cannot be built here; these
are outputs of oracle/magnetite_oracle.c and scipy.
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
from magnetite_amd import meshgen  # noqa: E402
from make_fullsize_fixtures import sample_indices  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RULES = {"rnorm": oracle.STOP_RNORM, "rnorm_sq": oracle.STOP_RNORM_SQ}
PARTS = ("direct",) + tuple(RULES)
MAX_REFINE = 10


def system(p, threads=8):
    K = oracle.assemble_sparse(p.xy_flat, p.conn_flat, p.poisson_ratio, p.youngs_modulus, p.part_thickness,
                               threads=threads)
    A, b = oracle.reduce_system(K, p.u_known, p.u_in, p.f_in)
    return K, A, b


def scipy_csr(A):
    import scipy.sparse as sp
    return sp.csr_matrix((A.val, A.col, A.rowptr), shape=(A.n, A.n))


def direct_solve(A, b):
    """splu + iterative refinement until the step stops shrinking.  Returns x, the relative true residual, the relative
    size of the last step taken, and the number of steps."""
    from scipy.sparse.linalg import splu
    lu = splu(scipy_csr(A).tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0,
              options=dict(SymmetricMode=True))
    x = lu.solve(b)
    last, steps = np.inf, 0
    for _ in range(MAX_REFINE):
        dx = lu.solve(b - A.spmv(x))
        step = float(np.linalg.norm(dx) / np.linalg.norm(x))
        if step >= last:
            break
        x, last, steps = x + dx, step, steps + 1
    return x, float(np.linalg.norm(b - A.spmv(x)) / np.linalg.norm(b)), last, steps


def part(name, which, tmp):
    p = meshgen.baseline_problem(name)
    _, A, b = system(p)
    t0 = time.time()
    if which == "direct":
        x, res, step, steps = direct_solve(A, b)
        np.savez(os.path.join(tmp, f"{name}_{which}.npz"), x=x, rel_residual=res, last_step=step, steps=steps)
    else:
        x, it, cost, _ = oracle.cg(A, b, stop_mode=RULES[which], tol=oracle.TARGET_CG_COST)
        np.savez(os.path.join(tmp, f"{name}_{which}.npz"), x=x, iterations=it, final_cost=cost)
    print(f"{name} {which}: {time.time() - t0:.0f} s", flush=True)


def derived(p, K, x):
    """u, f, stress of a free-DOF solution x, as orc_run_sparse forms them."""
    known = p.u_known == 1
    u = p.u_in.copy()
    u[~known] = x
    f = p.f_in.copy()
    f[known] = K.spmv(u)[known]
    return u, f, oracle.stress(p.xy_flat, p.conn_flat, u, p.poisson_ratio, p.youngs_modulus)


def merge(name, tmp):
    p = meshgen.baseline_problem(name)
    N, E = p.mesh.num_nodes, p.mesh.num_elements
    K, A, b = system(p)
    known = p.u_known == 1
    iu, ie = sample_indices(2 * N), sample_indices(E)
    bn = float(np.linalg.norm(b))
    d = np.load(os.path.join(tmp, f"{name}_direct.npz"))
    xd = d["x"]
    fields = dict(workload=name, num_nodes=N, num_elements=E, n_free=A.n, nnz_ff=A.nnz, b_norm=bn,
                  target_cost=oracle.TARGET_CG_COST, dof_idx=iu.astype(np.int32), elem_idx=ie.astype(np.int32),
                  xy_checksum=float(np.sum(p.xy_flat * np.arange(1, 2 * N + 1) % 7.0)),
                  conn_checksum=int(np.sum(p.conn_flat.astype(np.int64) * (np.arange(3 * E) % 11 + 1))),
                  direct_solver="scipy splu (MMD_AT_PLUS_A, SymmetricMode, diag_pivot_thresh=0) + refinement",
                  direct_rel_residual=float(d["rel_residual"]), direct_last_step=float(d["last_step"]),
                  direct_refinement_steps=int(d["steps"]))

    def put(prefix, x):
        u, f, s = derived(p, K, x)
        fields.update({f"{prefix}_u_norm": np.linalg.norm(u), f"{prefix}_u_absmax": np.abs(u).max(),
                       f"{prefix}_f_known_norm": np.linalg.norm(f[known]), f"{prefix}_stress_norm": np.linalg.norm(s),
                       f"{prefix}_u_at": u[iu], f"{prefix}_f_at": f[iu], f"{prefix}_stress_at": s[ie]})

    put("direct", xd)
    for rule in RULES:
        c = np.load(os.path.join(tmp, f"{name}_{rule}.npz"))
        x = c["x"]
        r = float(np.linalg.norm(b - A.spmv(x)))
        fields.update({f"{rule}_solver": "orc_cg (1 thread)", f"{rule}_iterations": int(c["iterations"]),
                       f"{rule}_final_cost": float(c["final_cost"]),
                       f"{rule}_true_abs_residual": r, f"{rule}_true_rel_residual": r / bn,
                       f"{rule}_rel_l2_to_direct": float(np.linalg.norm(x - xd) / np.linalg.norm(xd))})
        put(rule, x)
    out = os.path.join(HERE, f"roundoff_{name}.npz")
    np.savez_compressed(out, **fields)
    print(f"{name}: E={E} n_free={A.n} direct: residual {fields['direct_rel_residual']:.2e} last step "
          f"{fields['direct_last_step']:.2e} ({fields['direct_refinement_steps']} steps)")
    for rule in RULES:
        print(f"  {rule}: iterations={fields[rule + '_iterations']} cost={fields[rule + '_final_cost']:.3e} "
              f"true residual {fields[rule + '_true_abs_residual']:.3e} abs {fields[rule + '_true_rel_residual']:.2e} rel, "
              f"to direct {fields[rule + '_rel_l2_to_direct']:.2e}")
    print(f"  -> {out} ({os.path.getsize(out) / 1024:.0f} KB)", flush=True)


def main(names):
    oracle.build()  # once, before the children would race to
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
        jobs = [(n, w, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--part", n, w, tmp], env=env))
                for n in names for w in PARTS]
        for n, w, j in jobs:
            if j.wait() != 0:
                raise SystemExit(f"{n} {w}: exit status {j.returncode}")
        for n in names:
            merge(n, tmp)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--part"]:
        part(*sys.argv[2:5])
    else:
        main(sys.argv[1:] or ["hole1m", "frontal1m"])
