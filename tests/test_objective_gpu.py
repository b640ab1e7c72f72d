"""GPU: mag_run_objective -- J, dJ/du and the explicit partials of both objectives against the reference module evaluated at the
DEVICE's u, for runs, load cases and variants; the same bits on a repeat, alone or in a chunk, staged or gathered; with the
adjoint, the results of Context.adjoint(g) bit for bit and totals that are one addition; the total gradient against the finite
differences a user would take with variants; and nothing else of the context changes."""
import numpy as np
import pytest

import adjoint_ref as aref
import objective_ref as oref
from load_cases_util import case_problem, make_cases
from magnetite_amd import Context, meshgen
from magnetite_amd.solver import MagnetiteError
from test_adjoint_gpu import assert_same_bits as assert_same_adjoint_bits
from test_adjoint_gpu import assert_stats_equal, stats_without_times
from test_load_cases_gpu import MESHES, TOL_F, rel
from test_member_sets_gpu import tensile
from test_sensitivities import base_problem
from variants_util import make_variants

pytestmark = pytest.mark.gpu

MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
KINDS = ("stress_pnorm", "disp_lsq")
PARITY = {
    "plate16": MESHES["plate16"][0],  # 289 nodes: one tile
    "tensile": tensile,  # 559 nodes
    "holes3k": MESHES["holes3k"][0],  # 3064 nodes: six tiles, halos
    "frontal516": lambda: meshgen.config_fixed_left_pull_right(meshgen.frontal_like(20, 0.4, 1)),  # a node of nine triangles
    "clockwise": lambda: meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24))),  # negative signed areas
}
VECTORS = ("g", "pxy")
SCALARS = ("J", "pJ_pE", "pJ_pnu", "pJ_pt")
TOTALS = ("dJ_dE", "dJ_dnu", "dJ_dt")


def spec_for(kind, prob, u, seed=6, members=None):
    """The objective's arguments for a problem solved to u: a weighted p = 8 aggregate whose scale is the largest von Mises stress
    at u (a typical stress, as the header asks); a least-squares mismatch on a node patch against a target off u.  With `members`,
    a row of weights (and of the target) per member."""
    rng = np.random.default_rng(seed)
    conn = np.asarray(prob.mesh.conn).reshape(-1, 3)
    rows = () if members is None else (members,)
    if kind == "stress_pnorm":
        sig = oref.element_stress(np.asarray(prob.mesh.xy).reshape(-1, 2), conn, u, prob.poisson_ratio, prob.youngs_modulus)
        return dict(weights=rng.uniform(0.5, 1.5, rows + (len(conn),)), p=8.0, scale=float(np.sqrt(oref.von_mises_sq(sig)).max()))
    w = aref.patch_weights(prob) * rng.uniform(0.5, 1.5, rows + (u.size,))
    return dict(weights=w, target=0.7 * u + 0.1 * np.abs(u).max() * rng.standard_normal(rows + (u.size,)))


def member_spec(spec, i):
    return {k: (v[i] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in spec.items()}


def assert_parity(what, got, want):
    """J, g, pxy and the explicit scalars at the same u: only round-off separates them.  rel <= 2 TOL_F for the first
    derivatives (the bar for products of strain-linear factors), J and dJ/dE = J / E relative to J, dJ/dnu within 2 TOL_F of the
    UN-CANCELLED sum of its element terms."""
    figures = {k: rel(got[k], want[k]) if np.abs(want[k]).max() > 0 else float(np.abs(got[k]).max()) for k in VECTORS}
    scal = {"J": abs(got["J"] - want["J"]) / want["J"], "pJ_pE": abs(got["pJ_pE"] - want["pJ_pE"]) / max(abs(want["pJ_pE"]), 1e-300),
            "pJ_pnu": abs(got["pJ_pnu"] - want["pJ_pnu"]) / max(want["pJ_pnu_abs"], 1e-300)}
    print(what, "rel", figures, "scalars", scal)
    assert want["J"] > 0 and np.abs(want["g"]).max() > 0
    for k in VECTORS:
        assert figures[k] <= 2 * TOL_F, (what, k)
    for k, v in scal.items():
        assert v <= 2 * TOL_F, (what, k, got[k], want[k])
    assert got["pJ_pt"] == 0.0


def assert_same_bits(a, b, what, keys=VECTORS, scalars=SCALARS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in scalars:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k, a[k], b[k])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_reference_at_the_devices_u(built, name, kind):
    prob = PARITY[name]()
    if name == "frontal516":
        assert np.bincount(np.asarray(prob.mesh.conn).reshape(-1)).max() >= 8
    with Context(device=0) as c:
        out = c.solve(prob)
        spec = spec_for(kind, prob, out["u"])
        got = c.objective(kind, "run", **spec)
    assert len(got) == 1 and "dxy" not in got[0]
    want = oref.of_problem(kind, prob, out["u"], **spec)
    if kind == "stress_pnorm":
        assert np.abs(want["pxy"]).max() > 0 and want["pJ_pnu"] != 0
    assert_parity((name, kind), got[0], want)


@pytest.mark.parametrize("per_member", [False, True], ids=["shared_rows", "member_rows"])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_for_cases_and_variants(built, kind, per_member):
    prob = PARITY["holes3k"]()
    M = 3
    xy, mat, u, f = make_variants(prob, M, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        spec = spec_for(kind, prob, outs[0]["u"], members=M if per_member else None)
        got = c.objective(kind, "variants", **spec)
        c.set_load_cases(u, f)
        c.run_cases()
        cases = [dict(u=c.download_case(i)[0]) for i in range(M)]
        got_cases = c.objective(kind, "cases", **spec)
        assert_same_bits(got[1], c.download_objective("variants", 1), "the variants' results outlive a run of the cases")
    assert len(got) == len(got_cases) == M
    for i in range(M):
        assert_parity(("variant", kind, i), got[i], oref.of_problem(kind, prob, outs[i]["u"], xy[i], mat[i], **member_spec(spec, i)))
        assert_parity(("case", kind, i), got_cases[i], oref.of_problem(kind, prob, cases[i]["u"], **member_spec(spec, i)))


def test_null_weights_are_ones_and_zero_stress_gives_zeros(built):
    prob = PARITY["plate16"]()
    E = len(prob.mesh.conn)
    idle = case_problem(prob, np.zeros_like(prob.u_in), np.zeros_like(prob.f_in))
    with Context(device=0) as c:
        out = c.solve(prob)
        scale = spec_for("stress_pnorm", prob, out["u"])["scale"]
        plain = c.objective("stress_pnorm", p=3.5, scale=scale)[0]
        ones = c.objective("stress_pnorm", weights=np.ones(E), p=3.5, scale=scale)[0]
        bare = c.objective("disp_lsq", weights=np.ones(out["u"].size))[0]
        assert c.solve(idle)["u"].any() == False  # noqa: E712 (u = 0: every element without stress)
        none = c.objective("stress_pnorm", p=1.0, scale=scale)[0]
    assert_same_bits(plain, ones, "weights")
    assert_parity("p = 3.5", plain, oref.of_problem("stress_pnorm", prob, out["u"], p=3.5, scale=scale))
    assert abs(bare["J"] - float(out["u"] @ out["u"])) <= 2 * TOL_F * bare["J"] and np.array_equal(bare["g"], 2.0 * out["u"])
    assert none["J"] == 0.0 and not none["g"].any() and not none["pxy"].any() and none["pJ_pnu"] == none["pJ_pE"] == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_a_repeat_and_a_member_alone_or_in_a_chunk_give_the_same_bits(built, monkeypatch, kind):
    monkeypatch.setenv("MAG_TUNE_SENS_CHUNK", "3")
    prob = PARITY["holes3k"]()
    V = 4
    xy, mat, u, f = make_variants(prob, V, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        spec = spec_for(kind, prob, outs[0]["u"], members=V)
        got = c.objective(kind, "variants", **spec)
        again = c.objective(kind, "variants", **spec)
    assert len({o["J"] for o in got}) == V
    for i in range(V):
        assert_same_bits(got[i], again[i], ("repeat", i))
    for i in (1, 3):  # inside the first chunk; the last chunk's only member
        with Context(device=0) as solo:
            solo.solve_variants(prob, xy[i:i + 1], mat[i:i + 1], u[i:i + 1], f[i:i + 1])
            alone = solo.objective(kind, "variants", **{k: (v[i:i + 1] if isinstance(v, np.ndarray) else v) for k, v in spec.items()})
        assert_same_bits(got[i], alone[0], ("solo", i))


@pytest.mark.parametrize("name", ["plate16", "holes3k", "frontal516"])
def test_tile_staging_and_the_gather_from_memory_give_the_same_bits(built, monkeypatch, name):
    prob = PARITY[name]()
    xy, mat, u, f = make_variants(prob, 2, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        spec = spec_for("stress_pnorm", prob, outs[0]["u"])
        staged = c.objective("stress_pnorm", "variants", **spec)
        monkeypatch.setenv("MAG_TUNE_SENS_STAGE", "0")
        plain = c.objective("stress_pnorm", "variants", **spec)
    for i in range(2):
        assert np.abs(staged[i]["g"]).max() > 0 and np.abs(staged[i]["pxy"]).max() > 0
        assert_same_bits(staged[i], plain[i], (name, i))


def scaled_to_the_rhs(c, kind, set, spec, prob, rhs_norms):
    """spec with every member's weights scaled so that |g_F| equals the member's primal right-hand side norm (g is linear in the
    least squares' weights and grows with w^(1/p) for the p-norm: there a factor c on g is a factor c^p on the
    weights): the default absolute stop rule then resolves the adjoint solve as it resolved the primal one."""
    first = c.objective(kind, set, **spec)
    free = prob.u_known == 0
    factors = np.array([r / np.linalg.norm(o["g"][free]) for o, r in zip(first, rhs_norms)]) ** spec.get("p", 1.0)
    w = spec["weights"]
    w = np.broadcast_to(w, (len(first),) + w.shape[-1:]) * factors[:, None]
    out = dict(spec, weights=np.ascontiguousarray(w))
    if "target" in out:
        out["target"] = np.ascontiguousarray(np.broadcast_to(out["target"], w.shape))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_with_the_adjoint_it_is_adjoint_of_g_bit_for_bit_and_totals_are_one_add(built, kind):
    prob = PARITY["holes3k"]()
    V = 3
    xy, mat, u, f = make_variants(prob, V, seed=11)
    with Context(device=0) as c:
        outs = c.solve_variants(prob, xy, mat, u, f)
        spec = scaled_to_the_rhs(c, kind, "variants", spec_for(kind, prob, outs[0]["u"]), prob, [o["rhs_norm"] for o in outs])
        plain = c.objective(kind, "variants", **spec)
        with pytest.raises(MagnetiteError) as e:  # no totals without the adjoint
            c.download_objective("variants", 0, total=True)
        assert e.value.code == MAG_ERR_STATE
        want = c.adjoint(np.stack([o["g"] for o in plain]), "variants")
        want_stats = [c.adjoint_stats("variants", i) for i in range(V)]
        want_info = c.adjoint_info("variants")
        got = c.objective(kind, "variants", adjoint=True, **spec)
        adj = [c.download_adjoint("variants", i) for i in range(V)]
        stats = [c.adjoint_stats("variants", i) for i in range(V)]
        assert c.adjoint_info("variants") == want_info
        with pytest.raises(MagnetiteError) as e:
            c.download_objective("variants", V)
        assert e.value.code == MAG_ERR_BAD_ARGS
    for i in range(V):
        assert stats[i]["converged"] == 1 and 0.1 <= stats[i]["rhs_norm"] / outs[i]["rhs_norm"] <= 10
        assert_same_bits(got[i], plain[i], ("explicit", i))
        assert_same_adjoint_bits(adj[i], want[i], ("adjoint", i))
        assert_stats_equal(stats[i], want_stats[i], ("adjoint stats", i))
        assert np.abs(adj[i]["dxy"]).max() > 0
        assert np.array_equal(got[i]["dxy"], got[i]["pxy"] + adj[i]["dxy"]), i
        for total, part in zip(TOTALS, SCALARS[1:]):
            assert np.float64(got[i][total]).tobytes() == np.float64(got[i][part] + adj[i][total]).tobytes(), (i, total)


@pytest.mark.parametrize("kind", KINDS)
def test_the_users_loop_finite_differences_through_variants(built, kind):
    """4 x 12 variants that move one coordinate by +-h and +-h/2: J of every variant from the device; the base variant's total
    dxy meets the inequality of the CPU tests against these differences."""
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
        spec = spec_for(kind, prob, outs[0]["u"])
        free = prob.u_known == 0
        g0 = c.objective(kind, "variants", **spec)[0]["g"]
        spec["weights"] = spec["weights"] * (outs[0]["rhs_norm"] / np.linalg.norm(g0[free])) ** spec.get("p", 1.0)  # (scaled_to_the_rhs)
        got = c.objective(kind, "variants", adjoint=True, **spec)
    g = got[0]["dxy"]
    gmax = np.abs(g).max()
    J = [o["J"] for o in got]
    for k, dof in enumerate(dofs):
        a = J[1 + 4 * k:5 + 4 * k]
        fd_h, fd_h2 = (a[0] - a[1]) / (2 * h), (a[2] - a[3]) / h
        err, rich = abs(g[dof] - fd_h2), abs(fd_h - fd_h2)
        print(kind, "dof", dof, "g", g[dof], "err/max|g|", err / gmax, "richardson/max|g|", rich / gmax)
        assert err <= 4 * rich + 2e-7 * gmax, dof


def test_it_leaves_everything_else_alone(built):
    prob = PARITY["holes3k"]()
    V = 3
    xy, mat, u, f = make_variants(prob, V, seed=4)
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.set_variants(xy, mat, u, f)
        c.run_variants()
        c.set_load_cases(u, f)
        c.run_cases()
        c.run()
        sets = ("variants", "cases", "run")
        members = dict(variants=V, cases=V, run=1)
        rhs = dict(variants=[c.variant_stats(i)["rhs_norm"] for i in range(V)], cases=[c.case_stats(i)["rhs_norm"] for i in range(V)],
                   run=[c.stats()["rhs_norm"]])
        u0 = c.download()[0]
        specs = {(k, s): scaled_to_the_rhs(c, k, s, spec_for(k, prob, u0), prob, rhs[s]) for k in KINDS for s in sets}
        for s in sets:
            c.run_sensitivities(s)
            c.adjoint(np.stack([o["g"] for o in c.objective("disp_lsq", s, **specs["disp_lsq", s])]), s)

        def record(skip_adjoint=None):
            out = dict(run=c.download(), run_stats=stats_without_times(c.stats()), cases_info=c.cases_info(),
                       variants_info=c.variants_info())
            for i in range(V):
                out["variant", i] = c.download_variant(i)
                out["variant_stats", i] = stats_without_times(c.variant_stats(i))
                out["case", i] = c.download_case(i)
                out["case_stats", i] = stats_without_times(c.case_stats(i))
            for s in sets:
                for i in range(members[s]):
                    out["sens", s, i] = c.download_sensitivity(s, i)
                    if s != skip_adjoint:
                        out["adjoint", s, i] = c.download_adjoint(s, i)
                        out["adjoint_stats", s, i] = stats_without_times(c.adjoint_stats(s, i))
                if s != skip_adjoint:
                    out["adjoint_info", s] = c.adjoint_info(s)
            return out

        def assert_unchanged(before, after, what):
            for key, a in after.items():
                b = before[key]
                if isinstance(b, tuple):
                    assert all(np.array_equal(x, y) for x, y in zip(a, b)), (what, key)
                elif key[0] in ("sens", "adjoint"):
                    for k in a:
                        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else \
                            np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, key, k)
                else:
                    assert a == b, (what, key, a, b)

        before = record()
        for kind in KINDS:
            for s in sets:
                got = c.objective(kind, s, **specs[kind, s])
                assert len(got) == members[s] and all(o["J"] > 0 for o in got)
                assert_unchanged(before, record(), (kind, s, "no adjoint"))
        for s in sets:  # with the adjoint: everything but the set's own adjoint results
            got = c.objective("stress_pnorm", s, adjoint=True, **specs["stress_pnorm", s])
            assert all(np.abs(o["dxy"]).max() > 0 for o in got)
            assert_unchanged(before, record(skip_adjoint=s), (s, "adjoint"))
            before = record()
        for s in sets:  # all three sets hold their objectives side by side
            c.download_objective(s, 0, total=True)
        # a new run of a set drops its objective (and, with the single-case results, that of "run"); the others stay
        c.run_cases()
        for s in ("cases", "run"):
            with pytest.raises(MagnetiteError) as e:
                c.download_objective(s, 0)
            assert e.value.code == MAG_ERR_STATE
        c.download_objective("variants", V - 1, total=True)
        c.set_variants(xy, mat, u, f)
        with pytest.raises(MagnetiteError) as e:
            c.download_objective("variants", 0)
        assert e.value.code == MAG_ERR_STATE
        c.run()
        c.objective("disp_lsq", "run", **specs["disp_lsq", "run"])
        c.upload_problem(prob)
        with pytest.raises(MagnetiteError) as e:
            c.download_objective("run", 0)
        assert e.value.code == MAG_ERR_STATE


def test_fall_back_one_member_after_another(built):
    prob = PARITY["holes3k"]()
    u, f = make_cases(prob, 3, seed=5)
    with Context(device=0, cg_variant=1) as c:
        outs = c.solve_cases(prob, u, f)
        spec = scaled_to_the_rhs(c, "stress_pnorm", "cases", spec_for("stress_pnorm", prob, outs[0]["u"]), prob,
                                 [o["rhs_norm"] for o in outs])
        got = c.objective("stress_pnorm", "cases", adjoint=True, **spec)
        info = c.adjoint_info("cases")
        adj = [c.download_adjoint("cases", i) for i in range(3)]
        want = c.adjoint(np.stack([o["g"] for o in got]), "cases")
    assert info[0] == 3 and info[1] == 0, info
    for i in range(3):
        assert_same_adjoint_bits(adj[i], want[i], ("adjoint", i))
        case = case_problem(prob, u[i], f[i])
        ref = oref.with_totals("stress_pnorm", case, outs[i]["u"], **member_spec(spec, i))
        assert_parity(("fall-back", i), got[i], ref)
        figure = rel(got[i]["dxy"], ref["dxy"])
        print("fall-back", i, "rel total dxy", figure)
        assert figure <= 2 * TOL_F, i
