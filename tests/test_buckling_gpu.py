"""GPU: mag_run_buckling -- the load factors of smallest magnitude and the buckling shapes of a solved member by subspace iteration
on the device -- against the dense factors of tests/buckling_ref.py; the geometric stiffness operator and its assembled form against
the scipy K_G, staged and gathered bit for bit; repeats bit for bit; the fall-back one vector after another, the gather walk, two
tile sizes; nothing else of the context changes; lifetime, refusals and the cap of outer steps.

Bars (from the issue; the modal tests' own): factors 1e-8 relative (the project's TOL_U), |Phi^T K Phi - I| 1e-10, true residual
1e-4 per mode, 1 - MAC (K inner product) of modes 1-4 1e-8, the operators 1e-14.  max_outer = 60 for every case.

Two settings the issue leaves open, and why they are what they are.  PRESTRESS: the reference factors come from a sparse-LU u0, so the
run that supplies u0 stops on a RELATIVE residual of 1e-12 -- the context's default rule is an absolute one (1e-4), which for
column16's loads of size 1 leaves u0, and with it every factor, at 3e-6 (measured: factor error 2.7e-6, true residual 1.2e-3).
INNER: the inner solves run to 1e-12 (the library's default is 1e-10), so that the factors' 1e-8 is no question of the inner solves.

K-orthonormality is measured against the stiffness assembled in extended precision, the products in extended precision
(buckling_ref.k_orthonormality): the float64 K of the twin is itself 1.4e-10 away from the stiffness in the quadratic form of the 16:1
column's shapes, which is what the device's shapes measured against it (1.7e-10), with and without the pass's last step.  That
step normalises the shapes once more by one matrix-free product K X; through A = Z^T Y alone they are K-orthonormal only as far as
the inner solves reach K Z = Y (1e-12 on the square parts, 1e-15 with the step; column16 against the stiffness itself: 8.7e-14)."""
import ctypes as C

import numpy as np
import pytest

import buckling_ref as ref
from device_buffers import DeviceArena
from magnetite_amd import Context, _lib
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import MESHES, TOL_U, rel
from test_modal_gpu import FOUR, clockwise_problem, same

pytestmark = pytest.mark.gpu

MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
OUTPUTS = ("load_factor", "residual", "shapes")
CAP = ref.MAX_OUTER
PRESTRESS = dict(stop_mode=_lib.MAG_STOP_REL, tol=1e-12)
INNER = dict(cg_tol=1e-12)


def assert_same_bits(a, b, what):
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), (what, k, rel(a[k], b[k]))
    for k in Context.BUCKLING_INFO:
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["critical"] == b["critical"], what


def check_factors(name, out):
    """every bar of the issue for one result of buckling() on part `name` of buckling_ref; returns the figures it printed"""
    prob, K, KG, free, u0, lam, Phi = ref.cached(name)
    p = len(out["load_factor"])
    assert p < len(lam)
    got, shapes = out["load_factor"], out["shapes"]
    err = float(np.max(np.abs(got - lam[:p]) / np.abs(lam[:p])))
    ortho = ref.k_orthonormality(ref.cached_stiffness_extended(name), shapes)  # (against the stiffness itself: buckling_ref says why)
    res = [ref.true_residual(K, KG, free, got[k], shapes[k]) for k in range(p)]
    mac = [1.0 - abs(float(Phi[k] @ (K @ shapes[k]))) for k in range(min(p, 4))]
    print(name, "p", p, "q", out["subspace"], "outer", out["outer"], "converged", out["converged"], "per launch", out["vectors_per_launch"], "launches",
          out["launches"], "redone", out["redone"], "factor err", err, "ortho", ortho, "true residual", max(res), "own residual",
          float(out["residual"].max()), "1-MAC", max(mac), "factors", got)
    assert out["converged"] == 1 and out["outer"] <= CAP
    assert np.all(np.diff(np.abs(got)) >= 0)  # by |lambda| ascending
    assert (np.sign(got) == np.sign(lam[:p])).all()
    assert err <= TOL_U
    assert ortho <= 1e-10
    assert max(res) <= 1e-4
    assert max(mac) <= 1e-8
    assert out["positive"] == int((lam[:p] > 0).sum())
    positive = got[got > 0]
    assert out["critical"] == (float(positive.min()) if positive.size else None)
    known = np.asarray(prob.u_known) != 0
    assert not shapes[:, known].any()
    for k in range(p):
        top = int(np.argmax(np.abs(shapes[k])))  # (the first of equals)
        assert shapes[k, top] > 0, (k, top)
    assert out["modes"] == p and out["residual"].shape == (p,) and np.all(out["residual"] >= 0) and np.all(out["residual"] <= 1e-3)
    return dict(err=err, ortho=ortho, res=max(res), mac=max(mac))


def csr_of(c, val):
    import scipy.sparse as sp
    rowptr, col, _ = c.assemble_csr()
    return sp.csr_matrix((val, col, rowptr), shape=(2 * c.N, 2 * c.N))


# ---- the operator

@pytest.mark.parametrize("name", FOUR)
def test_the_geometric_operator_and_its_assembled_form_against_the_twin(built, monkeypatch, name):
    prob = MESHES[name][0]()
    n2 = 2 * prob.mesh.num_nodes
    free = (np.asarray(prob.u_known) == 0).astype(np.float64)
    x = np.random.default_rng(5).uniform(-1.0, 1.0, n2)
    with Context(device=0) as c:
        u0 = c.solve(prob)["u"]
        plain, masked = c.apply_geometric(x), c.apply_geometric(x, masked=True)
        val = c.assemble_geometric()
        A = csr_of(c, val)
        with DeviceArena() as arena:  # device-resident output: the host path's bits
            out = arena.empty(val.size)
            rc = c._L.mag_assemble_geometric(c._h, _lib.MAG_SET_RUN, 0, C.cast(C.c_void_p(out.ptr), C.POINTER(C.c_double)), _lib.MAG_MEM_DEVICE)
            assert rc == 0, c._L.mag_last_error(c._h)
            arena.check()
            on_device = arena.read(out)
        monkeypatch.setenv("MAG_TUNE_SENS_STAGE", "0")
        plain0, masked0 = c.apply_geometric(x), c.apply_geometric(x, masked=True)
        again = c.assemble_geometric()
        after = c.download()[0]
    KG = ref.geometric_of(prob, u0)
    want, want_masked = KG @ x, free * (KG @ (free * x))
    entries = abs(A - KG).max() / abs(KG).max()
    print(name, "rel", rel(plain, want), "masked", rel(masked, want_masked), "entries", entries, "assembled against applied", rel(A @ x, plain))
    assert rel(plain, want) <= 1e-14
    assert rel(masked, want_masked) <= 1e-14
    assert np.array_equal(plain, plain0) and np.array_equal(masked, masked0)  # the staged walk and the gather: the same bits
    assert masked[free == 0].tolist() == [0.0] * int((free == 0).sum())
    assert entries <= 1e-14
    assert rel(A @ x, plain) <= 1e-14
    assert np.array_equal(on_device, val) and np.array_equal(again, val)
    coo = A.tocoo()
    assert not coo.data[coo.row % 2 != coo.col % 2].any()  # (h_kl I_2: the off-diagonal entries of every block are zeros)
    assert np.array_equal(after, u0)  # the run's result stays


def test_member_j_of_a_case_set_uses_that_cases_solution(built):
    prob = MESHES["plate16"][0]()
    n2 = 2 * prob.mesh.num_nodes
    rng = np.random.default_rng(9)
    u_in = np.stack([prob.u_in, 2.0 * prob.u_in, -0.5 * prob.u_in])
    f_in = np.stack([prob.f_in, prob.f_in + (np.asarray(prob.u_known) == 0) * rng.uniform(-1e5, 1e5, n2), 2.0 * prob.f_in])
    x = rng.uniform(-1.0, 1.0, n2)
    with Context(device=0) as c:
        c.solve_cases(prob, u_in, f_in)
        for j in range(3):
            uj = c.download_case(j)[0]
            KG = ref.geometric_of(prob, uj)
            y, val = c.apply_geometric(x, set="cases", member=j), c.assemble_geometric(set="cases", member=j)
            assert rel(y, KG @ x) <= 1e-14, j
            assert abs(csr_of(c, val) - KG).max() <= 1e-14 * abs(KG).max(), j
        with pytest.raises(MagnetiteError) as e:
            c.apply_geometric(x, set="cases", member=3)
        assert e.value.code == MAG_ERR_BAD_ARGS and "member 3" in e.value.message
        with pytest.raises(MagnetiteError) as e:
            c.apply_geometric(x)  # (the cases ran, the single run did not)
        assert e.value.code == MAG_ERR_STATE and "mag_run" in e.value.message


# ---- the factors

@pytest.mark.parametrize("name,p,q", ref.CASES)
def test_factors_against_the_dense_eigensolver(built, name, p, q):
    prob = ref.cached(name)[0]
    with Context(device=0, **PRESTRESS) as c:
        out = c.buckling(prob, modes=p, subspace=q, max_outer=CAP, **INNER)
        stats = [c.buckling_stats(j) for j in range(q)]
    check_factors(name, out)
    assert out["subspace"] == q
    assert all(st["converged"] == 1 and st["iterations"] > 0 for st in stats)
    if name == "frontal_mix":  # the negative fourth factor in its place
        assert np.allclose(out["load_factor"][:5], ref.FRONTAL_MIX, rtol=0, atol=5e-3) and out["load_factor"][3] < 0 and out["positive"] == 5
    if name == "holes_pull":
        assert out["critical"] is None and out["positive"] == 0 and np.all(out["load_factor"] < 0)
    if name.startswith("column"):
        assert out["positive"] == p and out["critical"] == out["load_factor"][0]


def test_the_columns_critical_load_against_euler(built):
    prob = ref.cached("column16")[0]
    with Context(device=0, **PRESTRESS) as c:
        out = c.buckling(prob, modes=1, subspace=8, max_outer=CAP, **INNER)
    ratio = out["critical"] / ref.euler_load(prob, 16.0, 1.0)
    print("critical / Euler", ratio)
    assert out["converged"] == 1
    assert 1.0 < ratio < 1.25  # (the twin: 1.216 -- linear triangles lock in bending)


def test_doubled_loads_as_a_second_case_give_half_the_factors(built):
    prob = ref.cached("frontal_push")[0]
    u_in, f_in = np.stack([prob.u_in, 2.0 * prob.u_in]), np.stack([prob.f_in, 2.0 * prob.f_in])
    with Context(device=0, **PRESTRESS) as c:
        c.solve_cases(prob, u_in, f_in)
        one = c.buckling(modes=4, subspace=12, set="cases", member=0, max_outer=CAP, **INNER)
        two = c.buckling(modes=4, subspace=12, set="cases", member=1, max_outer=CAP, **INNER)
    check_factors("frontal_push", one)
    assert two["converged"] == 1
    print("2 lambda(2 f) / lambda(f) - 1", 2.0 * two["load_factor"] / one["load_factor"] - 1.0)
    assert np.max(np.abs(2.0 * two["load_factor"] / one["load_factor"] - 1.0)) <= 1e-8


# ---- the paths

def test_fall_back_one_vector_after_another(built):
    prob = ref.cached("frontal_push")[0]
    with Context(device=0, cg_variant=1, **PRESTRESS) as c:
        out = c.buckling(prob, modes=4, subspace=12, max_outer=CAP, **INNER)
    assert out["vectors_per_launch"] == 0 and out["launches"] == 0
    check_factors("frontal_push", out)


def test_the_gather_walk_without_tile_local_tables(built):
    prob = ref.cached("column8")[0]
    with Context(device=0, op_variant=1, **PRESTRESS) as c:
        out = c.buckling(prob, modes=6, subspace=14, max_outer=CAP, **INNER)
    check_factors("column8", out)


@pytest.mark.parametrize("tile_nodes", [256, 512])
def test_two_tile_sizes(built, tile_nodes):
    prob = ref.cached("frontal_mix")[0]
    with Context(device=0, tile_nodes=tile_nodes, **PRESTRESS) as c:
        out = c.buckling(prob, modes=6, subspace=14, max_outer=CAP, **INNER)
    check_factors("frontal_mix", out)


def test_a_repeat_gives_the_same_bits(built):
    prob = ref.cached("frontal_mix")[0]
    with Context(device=0) as c:
        first = c.buckling(prob, modes=6, subspace=14, max_outer=CAP)
        again = c.buckling(modes=6, subspace=14, max_outer=CAP)
    with Context(device=0) as fresh:
        other = fresh.buckling(prob, modes=6, subspace=14, max_outer=CAP)
    assert_same_bits(first, again, "the same context")
    assert_same_bits(first, other, "a fresh context")


# ---- nothing else changes

def test_it_leaves_everything_else_alone(built):
    prob = ref.cached("holes_pull")[0]
    n2 = 2 * prob.mesh.num_nodes
    L = 3
    rng = np.random.default_rng(4)
    u_in = np.stack([prob.u_in * s for s in (1.0, 0.5, -1.5)])
    f_in = np.stack([prob.f_in + (np.asarray(prob.u_known) == 0) * rng.uniform(-1e4, 1e4, n2) for _ in range(L)])

    def no_times(st):
        return {k: v for k, v in st.items() if not k.startswith("ms_")}

    def everything(c):
        out = dict(run=c.download(), stats=no_times(c.stats()), history=c.history(5), run_stress=c.download_stress("run", 0),
                   run_sens=c.download_sensitivity("run", 0), modal=c.download_modal(), modal_info=c.modal_info())
        for i in range(L):
            out[i] = dict(case=c.download_case(i), case_stats=no_times(c.case_stats(i)), sens=c.download_sensitivity("cases", i))
        return out

    def compare(a, b):
        for x, y in zip(a["run"], b["run"]):
            assert np.array_equal(x, y)
        assert a["stats"] == b["stats"] and np.array_equal(a["history"], b["history"])
        same(a["run_stress"], b["run_stress"], "stress of the run")
        same(a["run_sens"], b["run_sens"], "sensitivities of the run")
        same(a["modal"], b["modal"], "the modes")
        assert a["modal_info"] == b["modal_info"]
        for i in range(L):
            for x, y in zip(a[i]["case"], b[i]["case"]):
                assert np.array_equal(x, y), i
            assert a[i]["case_stats"] == b[i]["case_stats"], i
            same(a[i]["sens"], b[i]["sens"], (i, "sens"))

    with Context(device=0, history_len=16) as c:
        c.solve_cases(prob, u_in, f_in)
        c.run()
        c.run_sensitivities("cases")
        c.run_sensitivities("run")
        c.run_stress("run")
        c.modal(modes=3, density=2700.0)
        before = everything(c)
        opts = (c.options.stop_mode, c.options.tol)
        of_run = c.buckling(modes=2, subspace=8, max_outer=CAP)
        compare(before, everything(c))
        of_case = c.buckling(modes=2, subspace=8, set="cases", member=2, max_outer=CAP)
        compare(before, everything(c))
        assert (c.options.stop_mode, c.options.tol) == opts
        assert of_run["converged"] == 1 and of_case["converged"] == 1
        assert np.all(of_run["load_factor"] < 0) and np.all(of_case["load_factor"] > 0)  # (case 2 pushes where the run pulls)
        # the shapes survive the other entry points
        c.modal(modes=3, density=2700.0)
        c.run()
        c.run_cases()
        kept = c.download_buckling()
        for k in OUTPUTS:
            assert np.array_equal(kept[k], of_case[k]), k
        c.upload_problem(prob)  # a new upload drops them
        for call in (c.download_buckling, c.buckling_info, lambda: c.buckling_stats(0)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE


# ---- lifetime and refusals

def test_refusals(built):
    x = None
    with Context(device=0) as c:
        prob = ref.cached("column8")[0]
        x = np.ones(2 * prob.mesh.num_nodes)
        c.upload_problem(prob)
        for call in (c.download_buckling, c.buckling_info, lambda: c.run_buckling(modes=2), lambda: c.apply_geometric(x), c.assemble_geometric,
                     lambda: c.run_buckling(modes=2, set="cases")):  # before any run
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE, call
        c.run()
        with pytest.raises(MagnetiteError) as e:
            c.run_buckling(modes=2, set="cases")  # the run is solved, the cases are not
        assert e.value.code == MAG_ERR_STATE and "mag_run_cases" in e.value.message
        with pytest.raises(MagnetiteError) as e:
            c.run_buckling(modes=2, member=1)
        assert e.value.code == MAG_ERR_BAD_ARGS and "member 1" in e.value.message
        with pytest.raises(MagnetiteError) as e:
            c.run_buckling(modes=2, subspace=8, max_outer=-1)
        assert e.value.code == MAG_ERR_BAD_ARGS
        out = c.buckling(modes=2, subspace=8, max_outer=CAP)
        assert out["converged"] == 1
        # a new upload drops the results
        c.upload_problem(prob)
        with pytest.raises(MagnetiteError) as e:
            c.download_buckling()
        assert e.value.code == MAG_ERR_STATE
        # a field
        c.run()
        c.set_element_scale(np.full(prob.mesh.num_elements, 0.5))
        for call in (lambda: c.run_buckling(modes=2), lambda: c.apply_geometric(x), c.assemble_geometric):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE and "field" in e.value.message, call
    with Context(device=0) as c:  # a clockwise mesh (it solves: -K u = -f), the element named
        c.solve(clockwise_problem())
        with pytest.raises(MagnetiteError) as e:
            c.run_buckling(modes=2)
        assert e.value.code == MAG_ERR_BAD_ARGS and "mag_run_buckling: element 0 " in e.value.message
    with Context(device=0) as c:  # all-zero loads: no stress, nothing to buckle
        prob = ref.cached("column8")[0]
        c.upload(prob.xy_flat, prob.mesh.conn, prob.u_known, np.zeros_like(prob.u_in), np.zeros_like(prob.f_in), prob.youngs_modulus,
                 prob.poisson_ratio, prob.part_thickness)
        c.run()
        with pytest.raises(MagnetiteError) as e:
            c.run_buckling(modes=2)
        assert e.value.code == MAG_ERR_STATE and "prestress vanishes" in e.value.message and "carries no stress" in e.value.message
        with pytest.raises(MagnetiteError) as e:
            c.download_buckling()
        assert e.value.code == MAG_ERR_STATE


def test_the_cap_of_outer_steps_is_no_error(built):
    prob = ref.cached("holes_pull")[0]
    with Context(device=0) as c:
        out = c.buckling(prob, modes=4, subspace=12, max_outer=2)
        message = c._L.mag_last_error(c._h).decode()
    assert out["converged"] == 0 and out["outer"] == 2
    assert "mag_run_buckling stopped at the cap of 2 outer steps" in message
    assert np.all(np.isfinite(out["shapes"])) and np.all(np.isfinite(out["load_factor"])) and np.all(out["load_factor"] < 0)
