"""GPU: mag_run_adjoint -- the adjoint solves through the member-set driver and the bilinear pass -- against the reference module
applied to the ORACLE's solution and the twin's direct lambda; lambda bit for bit the load case / variant (0, g); batched members
bit for bit their solo runs; the gradient against the finite differences a user would take with variants; and nothing else of
the context changes."""
import functools

import numpy as np
import pytest

import adjoint_ref as aref
from load_cases_util import case_problem, make_cases
from magnetite_amd import Context, meshgen
from magnetite_amd._lib import MAG_OP_CSR
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import BITWISE_STATS, MESHES, TOL_F, TOL_U, assert_case_equals, rel
from test_sensitivities import base_problem
from variants_util import make_variants

pytestmark = pytest.mark.gpu

MAG_ERR_STATE = 7
PARITY = dict(MESHES)
del PARITY["plate100k"]
PARITY["clockwise"] = (lambda: meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24))), 1)
ARRAYS = ("lambda", "dloads", "delem", "dxy")


def weights(prob, u, rhs_norm):
    """J1's weights, scaled so that |g_F| = |2 w u|_F equals the primal right-hand side's norm: the default absolute stop rule
    then resolves the adjoint solve as it resolved the primal one."""
    w = aref.patch_weights(prob)
    g = aref.dJ1(w, u)[prob.u_known == 0]
    return w * (rhs_norm / np.linalg.norm(g))


def gradients(prob, outs):
    """(members, 2N): dJ1/du of every solved member at its own u, each member's weights scaled to its own right-hand side."""
    return np.stack([aref.dJ1(weights(prob, o["u"], o["rhs_norm"]), o["u"]) for o in outs])


def assert_same_bits(a, b, what):
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in aref.SCALARS:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k, a[k], b[k])


def assert_stats_equal(a, b, what):
    for key in BITWISE_STATS:
        assert a[key] == b[key], (what, key, a[key], b[key])
    for key in ("final_cost", "rhs_norm"):
        assert np.float64(a[key]).tobytes() == np.float64(b[key]).tobytes(), (what, key)


def oracle_u(prob, u_in=None, f_in=None):
    import oracle
    return oracle.run(prob.xy_flat, prob.conn_flat, prob.u_known, prob.u_in if u_in is None else u_in,
                      prob.f_in if f_in is None else f_in, prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness,
                      path="sparse")["u"]


def assert_parity(what, got, want):
    """rel(lambda) <= TOL_U; rel <= 2 TOL_F for dloads, delem, dxy (products of two strain-linear factors, each within TOL_F);
    the scalars within 2 TOL_F of the UN-CANCELLED sum of |delem|, because a = sum of delem may cancel."""
    figures = {k: rel(got[k], want[k]) for k in ARRAYS}
    bar = 2 * TOL_F * float(np.abs(want["delem"]).sum())
    scal = {"a": abs(got["a"] - want["a"]), "dJ_dE": abs(got["dJ_dE"] - want["dJ_dE"]) * want["E"],
            "dJ_dnu": abs(got["dJ_dnu"] - want["dJ_dnu"]), "dJ_dt": abs(got["dJ_dt"] - want["dJ_dt"]) * want["t"]}
    print(what, "rel", figures, "scalars' errors / bar", {k: v / bar for k, v in scal.items()})
    assert figures["lambda"] <= TOL_U, what
    for k in ("dloads", "delem", "dxy"):
        assert figures[k] <= 2 * TOL_F, (what, k)
    for k, v in scal.items():  # (dJ/dE and dJ/dt are -a / E and -a / t: the bar in their units)
        assert v <= bar, (what, k, got[k], want[k])


def reference(prob, u_oracle, g):
    want = aref.of_problem(prob, u_oracle, g)
    want.update(E=prob.youngs_modulus, t=prob.part_thickness)
    return want


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_reference_on_the_oracles_solution(built, name):
    prob = PARITY[name][0]()
    with Context(device=0) as c:
        out = c.solve(prob)
        g = aref.dJ1(weights(prob, out["u"], out["rhs_norm"]), out["u"])
        got = c.adjoint(g, "run")
        st = c.adjoint_stats("run", 0)
    assert len(got) == 1
    ratio = st["rhs_norm"] / out["rhs_norm"]
    print(name, "N", prob.mesh.num_nodes, "adjoint iterations", st["iterations"], "primal", out["iterations"], "|g_F| / |b|", ratio)
    assert 0.1 <= ratio <= 10 and st["converged"] == 1
    assert_parity(name, got[0], reference(prob, oracle_u(prob), g))


def test_lambda_is_the_load_case_bit_for_bit(built):
    prob = MESHES["holes3k"][0]()
    u, f = make_cases(prob, 7, seed=11)
    with Context(device=0) as c:
        outs = c.solve_cases(prob, u, f)
        G = gradients(prob, outs)
        adj = c.adjoint(G, "cases")
        stats = [c.adjoint_stats("cases", i) for i in range(7)]
        info = c.adjoint_info("cases")
    with Context(device=0) as c:
        want = c.solve_cases(prob, np.zeros_like(G), G)
        want_info = c.cases_info()
    print("cases", info, [s["iterations"] for s in stats])
    assert info[0] == 7 and info[1] >= 2 and info == list(want_info.values())
    for i in range(7):
        assert np.array_equal(adj[i]["lambda"], want[i]["u"]), i
        assert_stats_equal(stats[i], want[i], ("case", i))


def test_lambda_is_the_variant_bit_for_bit(built):
    prob = MESHES["holes3k"][0]()
    xy, mat, u, f = make_variants(prob, 5, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        G = gradients(prob, outs)
        adj = c.adjoint(G, "variants")
        stats = [c.adjoint_stats("variants", i) for i in range(5)]
        info = c.adjoint_info("variants")
    with Context(device=0) as c:
        want = c.solve_variants(prob, xy, mat, np.zeros_like(G), G)
    print("variants", info, [s["iterations"] for s in stats])
    assert info[0] == 5 and info[1] >= 2
    for i in range(5):
        assert np.array_equal(adj[i]["lambda"], want[i]["u"]), i
        assert_stats_equal(stats[i], want[i], ("variant", i))


def test_batched_members_equal_their_solo_runs_and_a_repeat_bitwise(built, monkeypatch):
    monkeypatch.setenv("MAG_TUNE_SENS_CHUNK", "3")
    prob = MESHES["holes3k"][0]()
    V = 7
    xy, mat, u, f = make_variants(prob, V, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        G = gradients(prob, outs)
        adj = c.adjoint(G, "variants")
        again = c.adjoint(G, "variants")
    assert len(adj) == V and len({a["a"] for a in adj}) == V
    for i in range(V):
        assert_same_bits(adj[i], again[i], ("repeat", i))
    for i in (0, 2, 3, 6):  # a chunk's first and last member, the last chunk's only one
        with Context(device=0) as solo:
            solo.solve_variants(prob, xy[i:i + 1], mat[i:i + 1], u[i:i + 1], f[i:i + 1])
            assert_same_bits(adj[i], solo.adjoint(G[i:i + 1], "variants")[0], ("solo", i))


@pytest.mark.parametrize("name", ["plate16", "holes3k", "frontal3k", "two_fans"])
def test_tile_staging_and_the_gather_from_memory_give_the_same_bits(built, monkeypatch, name):
    prob = MESHES[name][0]()
    xy, mat, u, f = make_variants(prob, 2, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        G = gradients(prob, outs)
        staged = c.adjoint(G, "variants")
        monkeypatch.setenv("MAG_TUNE_SENS_STAGE", "0")
        plain = c.adjoint(G, "variants")
    for i in range(2):
        assert np.abs(staged[i]["dxy"]).max() > 0
        assert_same_bits(staged[i], plain[i], (name, i))


@functools.lru_cache(maxsize=None)
def fallback_cases():
    """holes3k, 3 cases: the problem, the loads and the oracle's u per case, computed once for both fall-back contexts."""
    prob = MESHES["holes3k"][0]()
    u, f = make_cases(prob, 3, seed=5)
    return prob, u, f, [oracle_u(prob, u[i], f[i]) for i in range(3)]


@pytest.mark.parametrize("opts", [dict(cg_variant=1), dict(cg_operator=MAG_OP_CSR)], ids=["cg_variant1", "csr_operator"])
def test_fall_backs_one_member_after_another(built, opts):
    prob, u, f, u_oracle = fallback_cases()
    with Context(device=0, **opts) as c:
        outs = c.solve_cases(prob, u, f)
        G = gradients(prob, outs)
        adj = c.adjoint(G, "cases")
        info = c.adjoint_info("cases")
    assert info[0] == 3 and info[1] == 0, info
    for i in range(3):
        case = case_problem(prob, u[i], f[i])
        assert_parity((opts, i), adj[i], reference(case, u_oracle[i], G[i]))


def test_the_users_loop_finite_differences_through_variants(built):
    """4 x 12 variants that move one coordinate by +-h and +-h/2: J1 from each variant's downloaded u; the base variant's adjoint
    dxy meets the inequality of the CPU test against these differences."""
    prob = base_problem(meshgen.config_fixed_left_pull_right)
    base = prob.xy_flat
    h = 1e-3 * 0.1
    rng = np.random.default_rng(2)
    dofs = rng.choice(base.size, 12, replace=False)
    xy = [base]
    for dof in dofs:
        for s in (h, -h, h / 2, -h / 2):
            v = base.copy()
            v[dof] += s
            xy.append(v)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, np.stack(xy))
        w = weights(prob, outs[0]["u"], outs[0]["rhs_norm"])
        G = np.stack([aref.dJ1(w, o["u"]) for o in outs])
        adj = c.adjoint(G, "variants")
    g = adj[0]["dxy"]
    gmax = np.abs(g).max()
    J = [aref.J1(w, o["u"]) for o in outs]
    for k, dof in enumerate(dofs):
        a = J[1 + 4 * k:5 + 4 * k]
        fd_h, fd_h2 = (a[0] - a[1]) / (2 * h), (a[2] - a[3]) / h
        err, rich = abs(g[dof] - fd_h2), abs(fd_h - fd_h2)
        print("dof", dof, "g", g[dof], "err/max|g|", err / gmax, "richardson/max|g|", rich / gmax)
        assert err <= 4 * rich + 2e-7 * gmax, dof


def stats_without_times(st):
    return {k: v for k, v in st.items() if not k.startswith("ms_")}


def test_it_leaves_everything_else_alone(built):
    prob = MESHES["holes3k"][0]()
    V = 3
    xy, mat, u, f = make_variants(prob, V, seed=4)
    with Context(device=0) as fresh:
        want_solve = fresh.solve(prob)
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.set_variants(xy, mat, u, f)
        c.run_variants()
        c.set_load_cases(u, f)
        c.run_cases()
        c.run()

        def record():
            out = dict(run=c.download(), run_stats=stats_without_times(c.stats()), cases_info=c.cases_info(),
                       variants_info=c.variants_info())
            for i in range(V):
                out["variant", i] = c.download_variant(i)
                out["variant_stats", i] = stats_without_times(c.variant_stats(i))
                out["case", i] = c.download_case(i)
                out["case_stats", i] = stats_without_times(c.case_stats(i))
                for s in ("cases", "variants"):
                    out["sens", s, i] = c.download_sensitivity(s, i)
            out["sens", "run", 0] = c.download_sensitivity("run", 0)
            return out

        def assert_unchanged(before, after, what):
            assert before.keys() == after.keys()
            for key, b in before.items():
                a = after[key]
                if isinstance(b, tuple):
                    assert all(np.array_equal(x, y) for x, y in zip(a, b)), (what, key)
                elif key[0] == "sens":
                    assert np.array_equal(a["energy"], b["energy"]) and np.array_equal(a["dxy"], b["dxy"]), (what, key)
                    assert all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in a if np.isscalar(a[k])), (what, key)
                else:
                    assert a == b, (what, key, a, b)

        for s in ("variants", "cases", "run"):
            c.run_sensitivities(s)
        before = record()
        G = {"run": gradients(prob, [dict(u=before["run"][0], rhs_norm=c.stats()["rhs_norm"])])[0],
             "cases": gradients(prob, [dict(u=before["case", i][0], rhs_norm=c.case_stats(i)["rhs_norm"]) for i in range(V)]),
             "variants": gradients(prob, [dict(u=before["variant", i][0], rhs_norm=c.variant_stats(i)["rhs_norm"]) for i in range(V)])}
        for s in ("variants", "cases", "run"):
            got = c.adjoint(G[s], s)
            assert len(got) == (1 if s == "run" else V) and all(np.abs(a["dxy"]).max() > 0 for a in got)
            assert_unchanged(before, record(), s)
        # for "run", sensitivities("run") still answers, with the same bits
        again = c.sensitivities("run")[0]
        assert np.array_equal(again["dxy"], before["sens", "run", 0]["dxy"])
        for s in ("variants", "cases", "run"):  # all three sets hold their adjoints side by side
            c.download_adjoint(s, 0)
        with pytest.raises(MagnetiteError):
            c.download_adjoint("cases", V)
        # a new run of a set drops its adjoint (and, with the single-case results, that of "run"); the others stay
        c.run_cases()
        for s in ("cases", "run"):
            with pytest.raises(MagnetiteError) as e:
                c.download_adjoint(s, 0)
            assert e.value.code == MAG_ERR_STATE
            with pytest.raises(MagnetiteError) as e:
                c.adjoint_info(s)
            assert e.value.code == MAG_ERR_STATE
        c.download_adjoint("variants", V - 1)
        # a new upload drops all three; a plain solve afterwards is a fresh context's
        assert_case_equals(c.solve(prob), want_solve, "plain solve afterwards")
        for s in ("variants", "cases", "run"):
            with pytest.raises(MagnetiteError) as e:
                c.download_adjoint(s, 0)
            assert e.value.code == MAG_ERR_STATE
        c.adjoint(G["run"], "run")
        c.run()
        with pytest.raises(MagnetiteError) as e:
            c.download_adjoint("run", 0)
        assert e.value.code == MAG_ERR_STATE


def test_self_adjoint_case_equals_the_energy_sensitivities(built):
    """Prescribed displacements all zero and g = f_in on the free DOFs: the adjoint system IS the primal one -- lambda = u bit for
    bit -- and dxy = -2 x the energy gradient of mag_run_sensitivities."""
    prob = meshgen.config_fixed_left_point_load(meshgen.plate(16))
    assert not prob.u_in.any()
    g = np.where(prob.u_known == 0, prob.f_in, 0.0)
    with Context(device=0) as c:
        out = c.solve(prob)
        sens = c.sensitivities("run")[0]
        adj = c.adjoint(g)[0]
    assert np.array_equal(adj["lambda"], out["u"])
    dmax = np.abs(sens["dxy"]).max()
    print("max |dxy + 2 dPi/dxy| / max|dxy|", np.abs(adj["dxy"] + 2 * sens["dxy"]).max() / dmax)
    assert np.abs(adj["dxy"] + 2 * sens["dxy"]).max() <= 1e-12 * dmax
    assert np.abs(adj["delem"] + 2 * sens["energy"]).max() <= 1e-12 * np.abs(sens["energy"]).max()
    assert abs(adj["a"] - 2 * sens["strain_energy"]) <= 1e-12 * abs(sens["strain_energy"])
