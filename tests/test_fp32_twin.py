"""CPU: the float32 twin of the fp32 CG leg (tests/fp32_twin.py) and the power of the operator probe the GPU tests use.

The twin in float64 must be the reference's operator and iteration; its float32 family must satisfy the probe's
precondition on every case of the GPU matrix; and errors seeded into a float32 realisation -- one row of K off by 1e-4, nu
off by 1e-4, coordinates cast before the origin is subtracted, an origin 30 extents away -- must stand at least twice above
the bar the GPU test will use (4 x the family maximum), or the case has no place in the matrix (fp32_cases lists those).
"""
import dataclasses

import numpy as np
import pytest

import fp32_cases as fc
import fp32_twin as tw
import numpy_twin
import oracle
from magnetite_amd import meshgen

SMALL = {
    "plate": lambda: meshgen.config_fixed_left_pull_right(meshgen.plate(7, 5, 1.4, 1.0)),
    "shuffled_load": lambda: meshgen.config_fixed_left_point_load(meshgen.shuffle(meshgen.plate(9), 1)),
    "hole_perturbed": lambda: meshgen.config_fixed_left_pull_right(
        meshgen.shuffle(meshgen.perturb(meshgen.plate_with_holes(14), 0.2), 2)),
    "clockwise": lambda: meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(8))),
    "zoo": lambda: fc.hold_rule(fc.zoo_mesh(np.random.default_rng(5)), 1e-9),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_float64_operator_is_the_reference_stiffness(name):
    p = SMALL[name]()
    Kd = numpy_twin.total_stiffness(p.mesh.xy, p.mesh.conn, p.poisson_ratio, p.youngs_modulus, p.part_thickness)
    free = (p.u_known == 0).astype(np.float64)
    n = Kd.shape[0]
    for origin, perm in tw.family(p, 3, seed=1):
        K = tw.apply(p, np.float64, origin=origin, element_perm=perm)
        got = np.stack([K(e) for e in np.eye(n)], axis=1)
        assert np.abs(got - free[:, None] * Kd).max() <= 1e-13 * np.abs(Kd).max()
        assert not got[p.u_known == 1].any()
    v = np.random.default_rng(3).standard_normal(n)
    assert np.abs(K(v) - free * (Kd @ v)).max() <= 1e-13 * (np.abs(Kd) @ np.abs(v)).max()


@pytest.mark.parametrize("name", ["plate24_shuffled", "hole_perturbed", "clockwise"])
def test_float64_history_follows_the_oracle(built, name):
    """the recurrence with beta one step ahead of its reduction, against argmin's as the oracle states them: the bar of the
    fp64 kernels' history assertions (test_full_solve_parity)"""
    p = {"plate24_shuffled": lambda: meshgen.config_fixed_left_point_load(meshgen.shuffle(meshgen.plate(24), 3)),
         "hole_perturbed": lambda: meshgen.config_fixed_left_pull_right(fc.hole_mesh()),
         "clockwise": lambda: meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24)))}[name]()
    ref = oracle.run(p.xy_flat, p.conn_flat, p.u_known, p.u_in, p.f_in, p.youngs_modulus, p.poisson_ratio,
                     p.part_thickness, path="sparse", hist_len=32, max_iter=32)
    K = tw.apply(p, np.float64)
    b = tw.rhs(p, fc.Csr64(p).matvec)
    s = tw.solve(p, K, b, np.float64, max_iter=32)
    assert s["iterations"] == ref["iterations"] == 32
    assert np.allclose(s["history"], ref["history"][:32], rtol=1e-9)
    assert s["best_iteration"] == int(np.argmin(ref["history"])) + 1
    assert np.linalg.norm(s["u"] - ref["u"]) <= 1e-9 * np.linalg.norm(ref["u"])  # both return best_param


def test_recurrence_bookkeeping(built):
    p = fc.problem("plate24_shuffled")
    K = tw.apply(p, np.float32)
    b = fc.reference("plate24_shuffled")["b"]
    one, two = tw.cg(K, b, np.float32, max_iter=1), tw.cg(K, b, np.float32, max_iter=2)
    assert one["iterations"] == 1 and one["best_iteration"] == 1 and len(one["history"]) == 1
    assert two["iterations"] == 2 and two["history"][0] == one["history"][0]
    # x1 = fl(alpha1 b): alpha1 read back from the iterate is the float32 alpha to a rounding
    x1 = one["x"]
    assert abs(float(x1 @ b) / float(b @ b) / one["alphas"][0] - 1.0) <= tw.EPS32
    z = tw.cg(K, np.zeros_like(b), np.float32)
    assert z["iterations"] == 0 and z["converged"] and not z["x"].any()
    rel = tw.cg(K, b, np.float32, stop_mode=tw.STOP_REL, tol=1e-3)
    assert rel["converged"] and rel["final_cost"] <= 1e-3 * np.linalg.norm(b) < rel["history"][-2]


@pytest.mark.parametrize("name", fc.CASES)
def test_family_meets_the_probe_precondition(built, name):
    """best_iteration == 2 in the solve capped at two iterations, for every member: d = u2 - u1 is then alpha2 p2"""
    fam = fc.family_probe(name)
    assert len(fam) == 8 and all(f[2] == 2 for f in fam)
    assert all(np.isfinite(f[0]) and f[0] > 0.0 for f in fam)
    p = fc.problem(name)
    assert not p.u_in.any()                                                   # only zero displacements are prescribed
    assert np.array_equal(p.f_in.astype(np.float32).astype(np.float64), p.f_in)  # b is exact in float32
    if name in fc.BAR_FROM:  # the transformed problem is the same problem: same topology, same loads
        src = fc.problem(fc.BAR_FROM[name])
        assert np.array_equal(src.mesh.conn, p.mesh.conn) and np.array_equal(src.f_in, p.f_in)


def typical_row(ref):
    """the free DOF whose |q_i| / (|K||b|)_i is the median: a row with neither unusually much nor little cancellation"""
    idx = np.where(ref["free"] & (ref["Kabs_b"] > 0.0))[0]
    frac = np.abs(ref["q_ref"][idx]) / ref["Kabs_b"][idx]
    return int(idx[np.argsort(frac)[len(idx) // 2]])


def seeded_errors(name):
    p, ref = fc.problem(name), fc.reference(name)
    lo, ext = p.mesh.xy.min(axis=0), np.ptp(p.mesh.xy, axis=0)
    K0, row = tw.apply(p, np.float32), typical_row(ref)

    def one_row_off(v):
        q = K0(v)
        q[row] *= np.float32(1.0 + 1e-4)
        return q

    nu = p.poisson_ratio
    wrong_nu = dataclasses.replace(p, poisson_ratio=nu * (1.0 + 1e-4) if nu else 1e-4)  # (absolute where nu = 0)
    far = dataclasses.replace(p, mesh=meshgen.Mesh(p.mesh.xy + 1e3 * ext, p.mesh.conn, "far"))
    return {"one row off by 1e-4": one_row_off,
            "nu off by 1e-4": tw.apply(wrong_nu, np.float32),
            "cast before subtract, 1e3 extents away": tw.apply(far, np.float32, origin=lo + 1e3 * ext, cast_first=True),
            "origin 30 extents away": tw.apply(p, np.float32, origin=lo - 30.0 * ext)}


@pytest.mark.parametrize("name", [n for n in fc.CASES if n not in fc.BAR_FROM])
def test_probe_separates_seeded_errors_from_the_family(built, name):
    p, ref = fc.problem(name), fc.reference(name)
    bar, _ = fc.bars(name)
    for what, K in seeded_errors(name).items():
        u1, two = fc.probe_pair(p, K, ref["b"])
        ratio, _ = fc.probe(name, u1, two["u"])
        print(f"{name}: {what}: ratio {ratio:.1f}, bar {bar:.1f}")
        assert two["best_iteration"] == 2
        assert ratio >= 2.0 * bar, (what, ratio, bar)
