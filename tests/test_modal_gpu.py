"""GPU: mag_run_modal -- the lowest natural frequencies and mode shapes of the uploaded part by subspace iteration on the device --
against scipy's shift-invert Lanczos on K and M assembled by tests/modal_ref.py; the mass operator against the scipy M, staged and
gathered bit for bit; repeats bit for bit; the fall-back one vector after another; nothing else of the context changes; lifetime,
refusals and the cap of outer steps.

Bars (from the issue; the reference alone is at 1e-11): eigenvalues 1e-8 relative (the project's TOL_U), |Phi^T M Phi - I| 1e-10,
true residual 1e-4 per mode, 1 - MAC of modes 1-4 1e-8, the mass operator 1e-14."""
import numpy as np
import pytest

import modal_ref as ref
from magnetite_amd import Context, meshgen
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import MESHES, TOL_U, assert_case_equals, rel
from variants_util import make_variants

pytestmark = pytest.mark.gpu

MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
RHO = 2700.0
FOUR = ("plate16", "holes3k", "frontal3k", "two_fans")
OUTPUTS = ("lambda", "frequency", "residual", "shapes")


def clockwise_problem():
    return meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24)))


def assert_same_bits(a, b, what):
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), (what, k, rel(a[k], b[k]))
    for k in Context.MODAL_INFO:
        assert a[k] == b[k], (what, k, a[k], b[k])


def check_modes(name, out, lumped=False, max_outer=40, pairs=8):
    """every bar of the issue for one result of modal() on part `name` of modal_ref.PARTS, against `pairs` (more than the modes
    of out) reference pairs; returns the figures it printed"""
    prob, K, M, free, lam, Phi = ref.cached(name, RHO, lumped, pairs)
    assert len(out["lambda"]) < pairs
    p = len(out["lambda"])
    shapes = out["shapes"]
    err = float(np.max(np.abs(out["lambda"] - lam[:p]) / lam[:p]))
    ortho = float(np.max(np.abs(shapes @ (M @ shapes.T) - np.eye(p))))
    res = [ref.true_residual(K, M, free, out["lambda"][k], shapes[k]) for k in range(p)]
    mac = [1.0 - abs(float(Phi[k] @ (M @ shapes[k]))) for k in range(min(p, 4))]
    print(name, "lumped" if lumped else "consistent", "outer", out["outer"], "converged", out["converged"], "per launch", out["vectors_per_launch"],
          "launches", out["launches"], "redone", out["redone"], "eig err", err, "ortho", ortho, "true residual", max(res), "own residual",
          float(out["residual"].max()), "1-MAC", max(mac), "Hz", out["frequency"])
    assert out["converged"] == 1 and out["outer"] <= max_outer
    assert np.all(np.diff(out["lambda"]) >= 0)
    assert err <= TOL_U
    assert ortho <= 1e-10
    assert max(res) <= 1e-4
    assert max(mac) <= 1e-8
    known = np.asarray(prob.u_known) != 0
    assert not shapes[:, known].any()
    for k in range(p):
        top = int(np.argmax(np.abs(shapes[k])))  # (the first of equals)
        assert shapes[k, top] > 0, (k, top)
    assert np.array_equal(out["frequency"], np.sqrt(out["lambda"]) / (2 * np.pi))
    assert out["modes"] == p and out["residual"].shape == (p,) and np.all(out["residual"] >= 0) and np.all(out["residual"] <= 1e-3)
    return dict(err=err, ortho=ortho, res=max(res), mac=max(mac))


@pytest.mark.parametrize("name", FOUR + ("clockwise",))
@pytest.mark.parametrize("lumped", [False, True])
def test_the_mass_operator_against_the_scipy_matrix(built, monkeypatch, name, lumped):
    prob = clockwise_problem() if name == "clockwise" else MESHES[name][0]()
    M = ref.mass(prob.mesh.xy, prob.mesh.conn, RHO, prob.part_thickness, lumped)
    free = (np.asarray(prob.u_known) == 0).astype(np.float64)
    x = np.random.default_rng(5).uniform(-1.0, 1.0, 2 * prob.mesh.num_nodes)
    with Context(device=0) as c:
        c.upload_problem(prob)
        plain, masked = c.apply_mass(x, RHO, lumped), c.apply_mass(x, RHO, lumped, masked=True)
        monkeypatch.setenv("MAG_TUNE_SENS_STAGE", "0")
        plain0, masked0 = c.apply_mass(x, RHO, lumped), c.apply_mass(x, RHO, lumped, masked=True)
    want, want_masked = M @ x, free * (M @ (free * x))
    print(name, lumped, "rel", rel(plain, want), "masked", rel(masked, want_masked))
    assert rel(plain, want) <= 1e-14
    assert rel(masked, want_masked) <= 1e-14
    assert np.array_equal(plain, plain0) and np.array_equal(masked, masked0)  # the staged walk and the gather: the same bits
    assert masked[free == 0].tolist() == [0.0] * int((free == 0).sum())


@pytest.mark.parametrize("name", FOUR)
def test_modes_against_shift_invert_lanczos(built, name):
    prob = MESHES[name][0]()
    with Context(device=0) as c:
        out = c.modal(prob, modes=6, density=RHO, max_outer=40)
        side_by_side = c.modal_info()["vectors_per_launch"]
        stats = [c.modal_stats(j) for j in range(out["subspace"])]
        c.set_load_cases(np.zeros((2, 2 * prob.mesh.num_nodes)), np.ones((2, 2 * prob.mesh.num_nodes)))
        c.run_cases()
        cases_per_launch = c.cases_info()["cases_per_launch"]
    check_modes(name, out)
    assert out["subspace"] == 12
    assert all(st["converged"] == 1 and st["iterations"] > 0 for st in stats)
    if cases_per_launch >= 2:  # where the load cases of this mesh run side by side, the vectors do
        assert side_by_side >= 2 and out["launches"] >= out["outer"] and out["redone"] == 0


def test_lumped_mass(built):
    prob = MESHES["holes3k"][0]()
    with Context(device=0) as c:
        lumped = c.modal(prob, modes=6, density=RHO, lumped=True, max_outer=40)
        consistent = c.modal(modes=6, density=RHO, max_outer=40)
    check_modes("holes3k", lumped, lumped=True)
    assert np.all(lumped["lambda"] < consistent["lambda"])


def test_a_repeat_gives_the_same_bits(built):
    prob = MESHES["holes3k"][0]()
    with Context(device=0) as c:
        first = c.modal(prob, modes=6, density=RHO)
        again = c.modal(modes=6, density=RHO)
    with Context(device=0) as fresh:
        other = fresh.modal(prob, modes=6, density=RHO)
    assert_same_bits(first, again, "the same context")
    assert_same_bits(first, other, "a fresh context")


def test_fall_back_one_vector_after_another(built):
    prob = MESHES["plate16"][0]()
    with Context(device=0, cg_variant=1) as c:
        out = c.modal(prob, modes=6, density=RHO, max_outer=40)
    assert out["vectors_per_launch"] == 0 and out["launches"] == 0
    check_modes("plate16", out)


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
    w = np.random.default_rng(8).uniform(0.5, 1.5, (V, 2 * prob.mesh.num_nodes))

    def no_times(st):
        return {k: v for k, v in st.items() if not k.startswith("ms_")}

    def everything(c):
        out = dict(run=c.download(), stats=no_times(c.stats()), history=c.history(5), run_stress=c.download_stress("run", 0),
                   run_sens=c.download_sensitivity("run", 0))
        for i in range(V):
            out[i] = dict(variant=c.download_variant(i), variant_stats=no_times(c.variant_stats(i)), case=c.download_case(i),
                          case_stats=no_times(c.case_stats(i)), sens=c.download_sensitivity("variants", i),
                          adjoint=c.download_adjoint("cases", i), adjoint_stats=no_times(c.adjoint_stats("cases", i)),
                          objective=c.download_objective("cases", i, total=True), stress=c.download_stress("variants", i))
        return out

    def compare(a, b):
        for x, y in zip(a["run"], b["run"]):
            assert np.array_equal(x, y)
        assert a["stats"] == b["stats"] and np.array_equal(a["history"], b["history"])
        same(a["run_stress"], b["run_stress"], "stress of the run")
        same(a["run_sens"], b["run_sens"], "sensitivities of the run")
        for i in range(V):
            for key in ("variant", "case"):
                for x, y in zip(a[i][key], b[i][key]):
                    assert np.array_equal(x, y), (i, key)
            for key in ("variant_stats", "case_stats", "adjoint_stats"):
                assert a[i][key] == b[i][key], (i, key)
            for key in ("sens", "adjoint", "objective", "stress"):
                same(a[i][key], b[i][key], (i, key))

    with Context(device=0, history_len=16) as c:
        c.solve_variants(prob, xy, mat, u, f)
        c.set_load_cases(u, f)
        c.run_cases()
        c.run()
        c.run_sensitivities("variants")
        c.run_sensitivities("run")
        c.run_objective("disp_lsq", "cases", weights=w, adjoint=True)
        c.run_stress("variants")
        c.run_stress("run")
        before = everything(c)
        opts = (c.options.stop_mode, c.options.tol)
        modes = c.modal(modes=4, density=RHO)
        assert modes["converged"] == 1
        compare(before, everything(c))
        # the modes survive the other entry points; a run afterwards is the run of a context that never saw them
        c.run()
        after_run = dict(zip(("u", "f", "stress"), c.download()), **c.stats())
        c.run_cases()
        kept = c.download_modal()
        for k in OUTPUTS:
            assert np.array_equal(kept[k], modes[k]), k
        c.upload_problem(prob)  # a new upload drops them
        for call in (c.download_modal, c.modal_info, lambda: c.modal_stats(0)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE
    with Context(device=0, history_len=16) as plain:
        assert (plain.options.stop_mode, plain.options.tol) == opts
        assert_case_equals(plain.solve(prob), after_run, "a solve that never saw the modal pass")


def test_refusals(built):
    with Context(device=0) as c:
        c.upload_problem(clockwise_problem())
        with pytest.raises(MagnetiteError) as e:
            c.run_modal(modes=2, density=RHO)
        assert e.value.code == MAG_ERR_BAD_ARGS and "element 0 " in e.value.message
        prob = MESHES["plate16"][0]()
        conn = prob.mesh.conn.copy()
        conn[37] = conn[37][[0, 2, 1]]
        c.upload(prob.xy_flat, conn, prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
        with pytest.raises(MagnetiteError) as e:
            c.run_modal(modes=2, density=RHO)
        assert e.value.code == MAG_ERR_BAD_ARGS and "element 37 " in e.value.message
        # three free DOFs only: subspace > n_free
        tiny = meshgen.plate(2)
        known = np.ones(2 * tiny.num_nodes, dtype=np.uint8)
        known[[8, 9, 10]] = 0
        c.upload(tiny.xy.reshape(-1), tiny.conn.reshape(-1), known, np.zeros(known.size), np.zeros(known.size), 7e10, 0.3, 0.5)
        with pytest.raises(MagnetiteError) as e:
            c.run_modal(modes=2, subspace=4, density=RHO)
        assert e.value.code == MAG_ERR_BAD_ARGS and "free DOFs" in e.value.message
        out = c.modal(modes=2, subspace=3, density=RHO)
        assert out["converged"] == 1 and np.all(out["lambda"] > 0)


def test_the_cap_of_outer_steps_is_no_error(built):
    prob = MESHES["plate16"][0]()
    with Context(device=0) as c:
        out = c.modal(prob, modes=6, density=RHO, max_outer=2)
    assert out["converged"] == 0 and out["outer"] == 2
    assert np.all(np.isfinite(out["shapes"])) and np.all(out["lambda"] > 0)
