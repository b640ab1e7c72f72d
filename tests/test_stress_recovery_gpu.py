"""GPU: mag_run_stress -- the stress tensor per element, the area-weighted nodal field, the ZZ error indicator and the scalars of
solved runs, load cases and design variants -- against the reference module applied to the u this context returned (round-off
only) and to the ORACLE's solution; batched members bit for bit their solo runs, tile staging bit for bit the gather from
memory; nothing else of the context changes; and sqrt(sum vm^2) is the objective pass's p = 2 aggregate."""
import functools

import numpy as np
import pytest

import stress_recovery_ref as ref
from load_cases_util import case_problem
from magnetite_amd import Context, meshgen
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import MESHES, TOL_F, assert_case_equals, rel
from variants_util import make_variants, variant_problem

pytestmark = pytest.mark.gpu

MAG_ERR_STATE = 7
PARITY = dict(MESHES)
del PARITY["plate100k"]
PARITY["clockwise"] = (lambda: meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24))), 1)
ROWS = ("elem", "node", "eta2")
SCALARS = ("eta", "energy_norm", "eta_rel", "vm_max", "vm_node_max")
# the binding's names -> the reference's: eta and energy_norm are the square roots of the library's sums
WANT = dict(eta=lambda w: np.sqrt(w["eta_sq"]), energy_norm=lambda w: np.sqrt(w["energy_sq"]), eta_rel=lambda w: w["eta_rel"],
            vm_max=lambda w: w["vm_max"], vm_node_max=lambda w: w["vm_node_max"])


def assert_same_bits(a, b, what):
    for k in ROWS:
        assert np.array_equal(a[k], b[k]), (what, k, rel(a[k], b[k]))
    for k in SCALARS:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k, a[k], b[k])


@functools.lru_cache(maxsize=None)
def solved(name):
    """The mesh's problem, what one context returned for it and the recovery of that run (solved once, shared, left unchanged)."""
    prob = PARITY[name][0]()
    with Context(device=0) as c:
        out = c.solve(prob)
        got = c.stress_recovery("run")
    assert len(got) == 1
    return prob, out, got[0]


@pytest.mark.parametrize("name", list(PARITY))
def test_arithmetic_of_the_pass_against_the_reference_on_the_returned_u(built, name):
    """Pure round-off: elem and node to 1e-12, eta2 to 1e-10 (the cancellation in sigma* - sigma_e, factor |sigma| / |d|),
    every scalar to 1e-10 relative."""
    prob, out, got = solved(name)
    want = ref.of_problem(prob, out["u"])
    print(name, "N", prob.mesh.num_nodes, "E", prob.mesh.num_elements, "cancellation |sigma|/|d|", ref.cancellation(want),
          {k: rel(got[k], want[k]) for k in ROWS}, {k: (got[k], float(WANT[k](want))) for k in SCALARS})
    assert got["elem"].shape == (prob.mesh.num_elements, 4) and got["node"].shape == (prob.mesh.num_nodes, 4)
    assert rel(got["elem"], want["elem"]) <= 1e-12
    assert rel(got["node"], want["node"]) <= 1e-12
    assert rel(got["eta2"], want["eta2"]) <= 1e-10
    for k in SCALARS:
        w = float(WANT[k](want))
        assert abs(got[k] - w) <= 1e-10 * abs(w), (k, got[k], w)
    assert got["energy_norm"] > 0 and (got["eta2"] >= 0).all()  # (|A|: on the clockwise mesh too)
    assert got["vm_max"] == got["elem"][:, 3].max() and got["vm_node_max"] == got["node"][:, 3].max()


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_reference_on_the_oracles_solution(built, name):
    """elem and node, linear in the strains, to the project's bar TOL_F.  eta2 and eta^2 amplify a difference in u by the
    cancellation in sigma* - sigma_e: d0, the distance between the reference on the oracle's u and the reference on the
    returned u, says by how much, and the device may be that far from the oracle-based value plus its own round-off."""
    import oracle
    prob, out, got = solved(name)
    sol = oracle.run(prob.xy_flat, prob.conn_flat, prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio,
                     prob.part_thickness, path="sparse")
    want, near = ref.of_problem(prob, sol["u"]), ref.of_problem(prob, out["u"])
    d0 = rel(near["eta2"], want["eta2"])
    d0_sum = abs(near["eta_sq"] - want["eta_sq"]) / want["eta_sq"]
    dist, dist_sum = rel(got["eta2"], want["eta2"]), abs(got["eta"] ** 2 - want["eta_sq"]) / want["eta_sq"]
    print(name, "rel elem", rel(got["elem"], want["elem"]), "rel node", rel(got["node"], want["node"]), "eta2: d0", d0, "device", dist,
          "eta^2: d0", d0_sum, "device", dist_sum)
    assert rel(got["elem"], want["elem"]) <= TOL_F
    assert rel(got["node"], want["node"]) <= TOL_F
    assert dist <= d0 + 1e-10
    assert dist_sum <= d0_sum + 1e-10


def test_batched_members_equal_their_solo_runs_bitwise(built, monkeypatch):
    monkeypatch.setenv("MAG_TUNE_SENS_CHUNK", "3")
    prob = MESHES["holes3k"][0]()
    V = 7
    xy, mat, u, f = make_variants(prob, V, seed=11)
    with Context(device=0) as c:
        c.solve_variants(prob, xy, mat, u, f)
        outs = c.stress_recovery("variants")
        again = c.stress_recovery("variants")
        c.solve_cases(prob, u, f)
        case_fields = c.stress_recovery("cases")
    assert len(outs) == V and len(case_fields) == V
    for i in range(V):
        assert_same_bits(outs[i], again[i], ("repeat", i))
    assert len({o["eta"] for o in outs}) == V
    for i in (0, 2, 3, 6):  # a chunk's first and last member, the last chunk's only one
        with Context(device=0) as solo:
            solo.solve_variants(prob, xy[i:i + 1], mat[i:i + 1], u[i:i + 1], f[i:i + 1])
            assert_same_bits(outs[i], solo.stress_recovery("variants")[0], ("solo", i))
    with Context(device=0) as fresh:  # variant 0 keeps the uploaded coordinates
        assert np.array_equal(xy[0], prob.xy_flat)
        fresh.solve(variant_problem(prob, None, mat[0], u[0], f[0]))
        assert_same_bits(outs[0], fresh.stress_recovery("run")[0], "uploaded coordinates")
    for i in (0, 1, 4, 6):
        with Context(device=0) as seq:
            seq.solve(case_problem(prob, u[i], f[i]))
            assert_same_bits(case_fields[i], seq.stress_recovery("run")[0], ("case", i))


@pytest.mark.parametrize("name", ["plate16", "holes3k", "frontal3k", "two_fans"])
def test_tile_staging_and_the_gather_from_memory_give_the_same_bits(built, monkeypatch, name):
    prob = MESHES[name][0]()
    xy, mat, u, f = make_variants(prob, 2, seed=11)
    with Context(device=0) as c:
        c.solve_variants(prob, xy, mat, u, f)
        staged = c.stress_recovery("variants")
        monkeypatch.setenv("MAG_TUNE_SENS_STAGE", "0")
        plain = c.stress_recovery("variants")
    for i in range(2):
        assert staged[i]["node"][:, 3].min() > 0 and staged[i]["eta"] > 0
        assert_same_bits(staged[i], plain[i], (name, i))


def same(a, b, what):
    """dicts of arrays and numbers, bit for bit"""
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k)


def test_it_leaves_everything_else_alone(built):
    prob = MESHES["holes3k"][0]()
    V = 3
    xy, mat, u, f = make_variants(prob, V, seed=4)
    rng = np.random.default_rng(8)
    w = rng.uniform(0.5, 1.5, (V, 2 * prob.mesh.num_nodes))

    def everything(c):
        out = []
        for i in range(V):
            st = {k: v for k, v in c.variant_stats(i).items() if not k.startswith("ms_")}
            out.append(dict(result=c.download_variant(i), stats=st, sens=c.download_sensitivity("variants", i),
                            adjoint=c.download_adjoint("variants", i), adjoint_stats={k: v for k, v in c.adjoint_stats("variants", i).items() if not k.startswith("ms_")},
                            objective=c.download_objective("variants", i, total=True)))
        return out

    with Context(device=0) as c:
        c.solve_variants(prob, xy, mat, u, f)
        c.run_sensitivities("variants")
        c.run_objective("disp_lsq", "variants", weights=w, adjoint=True)
        before = everything(c)
        fields = c.stress_recovery("variants")
        after = everything(c)
        for i in range(V):
            for a, b in zip(before[i]["result"], after[i]["result"]):
                assert np.array_equal(a, b), i
            assert before[i]["stats"] == after[i]["stats"] and before[i]["adjoint_stats"] == after[i]["adjoint_stats"], i
            for k in ("sens", "adjoint", "objective"):
                same(before[i][k], after[i][k], (i, k))
        # the other passes leave the recovery alone as well
        c.run_sensitivities("variants")
        c.run_objective("stress_pnorm", "variants", p=4.0, scale=fields[0]["vm_max"], adjoint=True)
        for i in range(V):
            assert_same_bits(c.download_stress("variants", i), fields[i], ("after the other passes", i))
        with pytest.raises(MagnetiteError):
            c.download_stress("variants", V)
        c.run_variants()  # a new run of the set drops its recovery
        with pytest.raises(MagnetiteError) as e:
            c.download_stress("variants", 0)
        assert e.value.code == MAG_ERR_STATE
        c.stress_recovery("variants")
        want_solve = c.solve(prob)  # a new upload drops it too
        for s in ("variants", "cases"):
            with pytest.raises(MagnetiteError) as e:
                c.download_stress(s, 0)
            assert e.value.code == MAG_ERR_STATE
        first = c.stress_recovery("run")[0]
        c.run()
        with pytest.raises(MagnetiteError) as e:
            c.download_stress("run", 0)
        assert e.value.code == MAG_ERR_STATE
        assert_same_bits(c.stress_recovery("run")[0], first, "the run again")
    with Context(device=0) as plain:
        assert_case_equals(plain.solve(prob), want_solve, "a solve that never saw the recovery")


@pytest.mark.parametrize("name", ["plate16", "holes3k"])
def test_the_objective_pass_aggregates_the_same_von_mises_stress(built, name):
    prob = MESHES[name][0]()
    with Context(device=0) as c:
        c.solve(prob)
        field = c.stress_recovery("run")[0]
        vm = field["elem"][:, 3]
        J = c.objective("stress_pnorm", "run", p=2.0, scale=float(vm.mean()))[0]["J"]
    l2 = float(np.sqrt(np.sum(vm * vm)))
    print(name, "sqrt(sum vm^2)", l2, "J", J, "rel", abs(J - l2) / l2)
    assert abs(J - l2) <= 1e-12 * l2
