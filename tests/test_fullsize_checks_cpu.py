"""CPU: the arbiters of the full-size GPU tests are themselves checked, where everything is cheap.

1. The oracle's CG (orc_cg, the thing every full-size fixture comes from) against a DIRECT solve of its own K_ff x = b
   (fullsize_checks.direct_solve: SuperLU + iterative refinement) on 10k-100k-triangle versions of the BASELINE
   workloads: three orders of magnitude above tests/numpy_twin.py, and not a CG.  Under the reference's stop rule they
   agree to 1.2e-12 (hole1m x 0.1), 7e-13 (frontal1m x 0.1), 1.1e-10 (plate100k) in rel-L2 of u; the bar is TOL_U = 1e-8.
2. tests/fullsize_checks.py passes on the oracle's own (u, f, stress) and FAILS on single mutations of a copy: the
   checks that tests/test_roundoff_parity_gpu.py runs on a million entries see one wrong entry.
3. The committed tests/golden/roundoff_*.npz are consistent with themselves and with the bars the GPU tests add their
   recorded distances to.
"""
import os

import numpy as np
import pytest

import fullsize_checks as fc
import oracle
from magnetite_amd import meshgen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_U = 1e-8
WORKLOADS = [("hole1m", 0.1), ("frontal1m", 0.1), ("plate100k", 1.0)]
_cache = {}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(params=WORKLOADS, ids=lambda w: w[0])
def solved(request, built):
    """(System, the oracle's run under the reference's stop rule) of a workload, once per module."""
    if request.param not in _cache:
        p = meshgen.baseline_problem(*request.param)
        ref = oracle.run(p.xy_flat, p.conn_flat, p.u_known, p.u_in, p.f_in, p.youngs_modulus, p.poisson_ratio,
                         p.part_thickness, path="sparse")
        _cache[request.param] = fc.System(p), ref
    return _cache[request.param]


def test_oracle_cg_against_a_direct_solve(solved):
    sys_, ref = solved
    A, b = oracle.reduce_system(sys_.K, sys_.p.u_known, sys_.p.u_in, sys_.p.f_in)
    x, residual, step = fc.direct_solve(A, b)
    # the arbiter's own error bar: a thousandth of what it arbitrates
    assert residual <= 1e-3 * TOL_U and step <= 1e-3 * TOL_U, (residual, step)
    d = rel(ref["u"][~sys_.known], x)
    print(f"{sys_.p.mesh.name}: n_free={A.n} iterations={ref['iterations']} oracle CG to direct solve {d:.2e} "
          f"(direct: residual {residual:.1e}, last step {step:.1e})")
    assert d <= TOL_U
    assert abs(sys_.residual(ref["u"]) - np.linalg.norm(b - A.spmv(ref["u"][~sys_.known])) / sys_.b_norm) <= 1e-3 * TOL_U


def test_checks_pass_on_the_oracles_own_result(solved):
    sys_, ref = solved
    own = sys_.residual(ref["u"])
    got = sys_.check_all(ref["u"], ref["f"], ref["stress"], residual_bar=4 * own)
    # the oracle's f and stress ARE these operations on its u: no round-off, nothing excluded
    assert got == dict(true_residual=own, residual_bar=4 * own, reaction_ratio=0.0, stress_mismatches=0)
    assert sys_.check_reactions(ref["u"], ref["f"], matrix_free=True) == 0.0


def _scale_one_free_u(s, u, f, st):
    u[np.flatnonzero(~s.known)[(~s.known).sum() // 2]] *= 1 + 1e-6


def _neighbours_reaction(s, u, f, st):
    k = np.flatnonzero(s.known)
    f[k[len(k) // 2]] = f[k[len(k) // 2 + 1]]


def _last_stress_is_first(s, u, f, st):
    st[-1] = st[0]


def _swap_two_blocks(s, u, f, st):
    a, b = u.size // 4, 3 * (u.size // 4)
    u[a:a + 512], u[b:b + 512] = u[b:b + 512].copy(), u[a:a + 512].copy()


def _free_f_one_ulp(s, u, f, st):
    i = np.flatnonzero(~s.known)[-1]
    f[i] = np.nextafter(f[i], np.inf)


# (mutation of a copy, the check that has to see it)
MUTATIONS = [(_scale_one_free_u, "residual"), (_neighbours_reaction, "reactions"), (_last_stress_is_first, "stress"),
             (_swap_two_blocks, "residual"), (_free_f_one_ulp, "reactions")]


@pytest.mark.parametrize("mutate,seen_by", MUTATIONS, ids=[m[0].__name__[1:] for m in MUTATIONS])
def test_checks_catch_a_single_mutation(solved, mutate, seen_by):
    sys_, ref = solved
    u, f, st = ref["u"].copy(), ref["f"].copy(), ref["stress"].copy()
    mutate(sys_, u, f, st)
    assert sum(not np.array_equal(a, ref[k]) for a, k in ((u, "u"), (f, "f"), (st, "stress"))) == 1
    bar = 4 * sys_.residual(ref["u"])
    check = {"residual": lambda: sys_.check_residual(u, bar), "reactions": lambda: sys_.check_reactions(u, f),
             "stress": lambda: sys_.check_stress(u, st)}[seen_by]
    with pytest.raises(AssertionError):
        check()
    with pytest.raises(AssertionError):
        sys_.check_all(u, f, st, residual_bar=bar)


@pytest.mark.parametrize("name", ["hole1m", "frontal1m"])
def test_roundoff_fixture_is_consistent(name):
    fx = np.load(os.path.join(GOLDEN, f"roundoff_{name}.npz"), allow_pickle=False)
    # the arbiter's own error bar: a thousandth of the displacement bar it arbitrates
    assert float(fx["direct_rel_residual"]) <= 1e-3 * TOL_U and float(fx["direct_last_step"]) <= 1e-3 * TOL_U
    for rule in ("rnorm", "rnorm_sq"):
        d = float(fx[f"{rule}_rel_l2_to_direct"])
        # the GPU test's bar against the direct solve is TOL_U + d: d has to stay the small part of it
        assert float(fx["direct_last_step"]) < d < TOL_U
        assert rel(fx[f"{rule}_u_at"], fx["direct_u_at"]) <= d
        assert abs(float(fx[f"{rule}_u_norm"]) - float(fx["direct_u_norm"])) <= d * float(fx["direct_u_norm"])
        assert float(fx[f"{rule}_true_rel_residual"]) * float(fx["b_norm"]) == pytest.approx(
            float(fx[f"{rule}_true_abs_residual"]), rel=1e-12)
        assert float(fx[f"{rule}_final_cost"]) <= float(fx["target_cost"])
    # the tighter rule iterates longer and lands closer
    assert int(fx["rnorm_iterations"]) > int(fx["rnorm_sq_iterations"]) > 1000
    assert float(fx["rnorm_rel_l2_to_direct"]) < float(fx["rnorm_sq_rel_l2_to_direct"])
