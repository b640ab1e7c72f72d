"""GPU: MAG_MEM_DEVICE on every entry point that takes a `memory` (include/magnetite_hip.h).  The reference is the same sequence of
calls with MAG_MEM_HOST on a second context with the same options: the device path adds copies, never arithmetic, so every
result agrees BIT FOR BIT -- there is no tolerance in this module; the host path is pinned to the oracle and the numpy twins by
the other modules.  Every caller's buffer lies between guard bands (tests/device_buffers.py) that are checked, with the inputs'
bytes, after every call; inputs are scribbled over once a call that copies them has returned.  Bad values that live on the
device are refused with the status, the message and the state left behind of their host twins."""
import contextlib

import numpy as np
import pytest

import design_ref as dref
import modal_ref
import refine_ref
import transient_ref
from device_buffers import UNWRITTEN, DeviceArena, Leg
from load_cases_util import make_cases
from magnetite_amd import Context
from magnetite_amd._lib import MAG_ERR_BAD_ARGS, MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import MESHES
from variants_util import make_variants

pytestmark = pytest.mark.gpu

MEMBERS = (0, 3, 6)  # of seven: the first, one in the middle, the last -- with chunks of three, the first of a chunk and a chunk's only one
RHO = 2700.0


@contextlib.contextmanager
def two_legs(offset=0, **options):
    """(host leg, device leg): two contexts with the same options, the device leg's arrays in an arena that is freed at the end"""
    with DeviceArena() as arena, Context(device=0, **options) as host, Context(device=0, **options) as dev:
        yield Leg(host, MAG_MEM_HOST), Leg(dev, MAG_MEM_DEVICE, arena, offset)
        arena.check()


def assert_same_bits(got, want, what):
    """dicts of arrays, scalars and words: shapes, types and bytes"""
    assert list(got) == list(want), (what, list(got), list(want))
    for k in got:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, k, int(np.count_nonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))), "bytes differ")


def written(out, what):
    """no array of a download is left as it was handed in, and none holds the scribble's NaNs"""
    for k, a in out.items():
        if isinstance(a, np.ndarray) and a.dtype == np.float64:
            assert np.isfinite(a).all(), (what, k)
    return out


def in_all_legs(legs, fn):
    host, dev = legs
    return fn(host), fn(dev)


# ---- load cases and variants ------------------------------------------------------------------------------------------------
def test_load_cases_from_device_memory_into_device_results(built):
    prob = MESHES["holes3k"][0]()
    u, f = make_cases(prob, 7, seed=3)
    with two_legs() as legs:
        def run(leg):
            leg.ctx.upload_problem(prob)
            assert leg.set_load_cases(u, f, scribble=True) == MAG_OK, leg.error()
            leg.ctx.run_cases()
            return {i: written(leg.download_case(i), ("case", i)) for i in MEMBERS}
        want, got = in_all_legs(legs, run)
        for i in MEMBERS:
            assert_same_bits(got[i], want[i], ("case", i))
            # ... and the device leg's results into host memory: inputs and outputs each on their own
            assert_same_bits(dict(zip(("u", "f", "stress"), legs[1].ctx.download_case(i))), want[i], ("case to the host", i))
        assert len({want[i]["u"].tobytes() for i in MEMBERS}) == len(MEMBERS)  # (an offset of 0 for every member would show)


@pytest.mark.parametrize("given", ["all", "xy", "material"])
def test_variants_from_device_memory_into_device_results(built, given):
    prob = MESHES["holes3k"][0]()
    xy, mat, u, f = make_variants(prob, 7, seed=11)
    args = dict(all=dict(xy=xy, material=mat, u_in=u, f_in=f), xy=dict(xy=xy), material=dict(material=mat))[given]
    with two_legs() as legs:
        def run(leg):
            leg.ctx.upload_problem(prob)
            assert leg.set_variants(7, scribble=True, **args) == MAG_OK, leg.error()
            leg.ctx.run_variants()
            return {i: written(leg.download_variant(i), ("variant", i)) for i in MEMBERS}
        want, got = in_all_legs(legs, run)
        for i in MEMBERS:
            assert_same_bits(got[i], want[i], (given, "variant", i))
            assert_same_bits(dict(zip(("u", "f", "stress"), legs[1].ctx.download_variant(i))), want[i], (given, "variant to the host", i))
        assert len({want[i]["u"].tobytes() for i in MEMBERS}) == len(MEMBERS)


# ---- the four derived passes: rows of a member out of the batched buffers ------------------------------------------------------
def solved_variants(leg, prob, V=7):
    xy, mat, u, f = make_variants(prob, V, seed=11)
    leg.ctx.upload_problem(prob)
    assert leg.set_variants(V, xy, mat, u, f) == MAG_OK, leg.error()
    leg.ctx.run_variants()
    leg.ctx.num_variants = V


def some_gradients(prob, M, seed=5):
    """dJ/du of the size of the right-hand side (the adjoint's stop rule): rows of random forces on the free DOFs"""
    rng = np.random.default_rng(seed)
    scale = max(float(np.abs(prob.f_in).max()), 1e3)
    return rng.standard_normal((M, prob.u_in.size)) * scale * 1e-2


def test_the_four_passes_download_device_rows_of_the_first_a_middle_and_the_last_member(built, monkeypatch):
    monkeypatch.setenv("MAG_TUNE_SENS_CHUNK", "3")  # members 0, 3 and 6 open a chunk, member 2 closes one
    prob = MESHES["holes3k"][0]()
    N, E = prob.mesh.num_nodes, prob.mesh.num_elements
    g = some_gradients(prob, 7)
    w = np.random.default_rng(2).uniform(0.5, 1.5, 2 * N)
    with two_legs() as legs:
        def run(leg):
            solved_variants(leg, prob)
            c = leg.ctx
            c.run_sensitivities("variants")
            c.run_stress("variants")
            assert leg.run_adjoint("variants", g) == MAG_OK, leg.error()
            out = {}
            for i in MEMBERS + (2,):
                out["sensitivity", i] = written(leg.download_sensitivity("variants", i), i)
                out["adjoint", i] = written(leg.download_adjoint("variants", i), i)
                out["stress", i] = written(leg.download_stress("variants", i), i)
                # NULL members stay skipped, the scalars are filled all the same
                out["sensitivity, dxy only", i] = leg.download_sensitivity("variants", i, want=("dxy",))
                out["adjoint, delem only", i] = leg.download_adjoint("variants", i, want=("delem",))
                out["adjoint, lambda and dxy", i] = leg.download_adjoint("variants", i, want=("lambda", "dxy"))
                out["stress, node only", i] = leg.download_stress("variants", i, want=("node",))
                out["stress, scalars only", i] = leg.download_stress("variants", i, want=())
                # the binding's own downloads, into host memory on either leg
                out["to the host", i] = dict(energy=c.download_sensitivity("variants", i)["energy"], delem=c.download_adjoint("variants", i)["delem"],
                                             eta2=c.download_stress("variants", i)["eta2"], scalars=out["stress", i]["scalars"])
            assert leg.run_objective("variants", "disp_lsq", weights=w, with_adjoint=0) == MAG_OK, leg.error()
            for i in MEMBERS:
                out["objective", i] = written(leg.download_objective("variants", i), i)
                out["objective, scalars only", i] = leg.download_objective("variants", i, want=())
            assert leg.run_objective("variants", "disp_lsq", weights=w, with_adjoint=1) == MAG_OK, leg.error()
            for i in MEMBERS:
                out["objective with totals", i] = written(leg.download_objective("variants", i, want=("g", "pxy", "dxy")), i)
                out["objective with totals, dxy only", i] = leg.download_objective("variants", i, want=("dxy",))
            return out
        want, got = in_all_legs(legs, run)
        assert list(got) == list(want)
        for key in want:
            assert_same_bits(got[key], want[key], key)
            assert np.isfinite(want[key]["scalars"]).all(), key  # always filled
        for name, part, full in (("sensitivity, dxy only", "dxy", "sensitivity"), ("adjoint, delem only", "delem", "adjoint"), ("stress, node only", "node", "stress")):
            for i in MEMBERS:
                assert list(got[name, i]) == [part, "scalars"]
                assert_same_bits(got[name, i], {k: got[full, i][k] for k in (part, "scalars")}, (name, i))
        for i in MEMBERS:
            assert want["objective", i]["scalars"][7] == 0.0 and want["objective with totals", i]["scalars"][7] == 1.0
        for what in ("sensitivity", "adjoint", "stress", "objective"):  # every member its own rows
            assert len({want[what, i]["scalars"].tobytes() for i in MEMBERS}) == len(MEMBERS), what
        for i in MEMBERS:  # device rows equal the rows the same context gives the host
            for name, key in (("sensitivity", "energy"), ("adjoint", "delem"), ("stress", "eta2")):
                assert np.array_equal(got["to the host", i][key], got[name, i][key]), (name, i)


@pytest.mark.parametrize("set", ["run", "cases", "variants"])
def test_run_adjoint_reads_its_rows_from_device_memory(built, monkeypatch, set):
    monkeypatch.setenv("MAG_TUNE_SENS_CHUNK", "3")
    prob = MESHES["holes3k"][0]()
    M = 1 if set == "run" else 7
    g = some_gradients(prob, M)
    with two_legs() as legs:
        def run(leg):
            if set == "run":
                leg.ctx.solve(prob)
            elif set == "cases":
                leg.ctx.upload_problem(prob)
                assert leg.set_load_cases(*make_cases(prob, M, seed=3)) == MAG_OK, leg.error()
                leg.ctx.run_cases()
            else:
                solved_variants(leg, prob)
            assert leg.run_adjoint(set, g, scribble=True) == MAG_OK, leg.error()
            return {i: written(leg.download_adjoint(set, i), (set, i)) for i in ((0,) if M == 1 else MEMBERS)}
        want, got = in_all_legs(legs, run)
        for i in want:
            assert_same_bits(got[i], want[i], (set, i))
            assert np.abs(want[i]["lambda"]).max() > 0
        assert len({o["lambda"].tobytes() for o in want.values()}) == len(want)


# ---- mag_run_objective: the caller's rows are read where they are, chunk after chunk -------------------------------------------
def objective_rows(kind, prob, M, stress):
    """weights and target, [M][2N] (disp_lsq) or weights [M][E] (stress_pnorm), every row its own; p and a typical stress"""
    rng = np.random.default_rng(9)
    N, E = prob.mesh.num_nodes, prob.mesh.num_elements
    if kind == "disp_lsq":
        return dict(weights=1e9 * rng.uniform(0.5, 1.5, (M, 2 * N)), target=1e-6 * rng.standard_normal((M, 2 * N)))
    return dict(weights=rng.uniform(0.5, 1.5, (M, E)), p=8.0, scale=float(np.abs(stress).max()))


def objective_combinations(kind, rows):
    """per_member 1 and 0 (the first row for all), with and without the target"""
    for per_member in (1, 0):
        spec = {k: (v if per_member or not isinstance(v, np.ndarray) else v[0]) for k, v in rows.items()}
        yield per_member, spec
        if kind == "disp_lsq":
            yield per_member, {k: v for k, v in spec.items() if k != "target"}


@pytest.mark.parametrize("offset", [0, 8], ids=["aligned", "on_8_bytes"])
@pytest.mark.parametrize("kind", ["disp_lsq", "stress_pnorm"])
def test_run_objective_reads_device_rows_in_place_chunk_by_chunk(built, monkeypatch, kind, offset):
    monkeypatch.setenv("MAG_TUNE_SENS_CHUNK", "3")  # 7 members: the launches start at rows 0, 3 and 6 of the caller's table
    prob = MESHES["holes3k"][0]()
    with two_legs(offset=offset) as legs:
        def run(leg):
            solved_variants(leg, prob)
            rows = objective_rows(kind, prob, 7, leg.ctx.download_variant(0)[2])
            out = {}
            for k, (per_member, spec) in enumerate(objective_combinations(kind, rows)):
                for with_adjoint in ((0, 1) if offset == 0 else (1,)):
                    # (_called: the rows read back unchanged after the call, and only then are they scribbled over)
                    assert leg.run_objective("variants", kind, per_member=per_member, with_adjoint=with_adjoint, **spec) == MAG_OK, leg.error()
                    want = ("g", "pxy", "dxy") if with_adjoint else ("g", "pxy")
                    for i in MEMBERS:
                        out[k, per_member, "target" in spec, with_adjoint, i] = written(leg.download_objective("variants", i, want=want), i)
                    if with_adjoint:
                        out[k, per_member, "target" in spec, "adjoint", 3] = leg.download_adjoint("variants", 3)
            for i in (3, 6):  # member i's own row as the one row of all members: what the table's row i must give member i
                assert leg.run_objective("variants", kind, per_member=0, **{k: (v[i] if isinstance(v, np.ndarray) else v) for k, v in rows.items()}) == MAG_OK
                out["row", i] = leg.download_objective("variants", i)
            return out
        want, got = in_all_legs(legs, run)
        assert list(got) == list(want) and len(want) >= (12 if offset == 0 else 8)
        for key in want:
            assert_same_bits(got[key], want[key], (kind, key))
        # the rows matter: with a row per member J differs from the shared row's for every member but the first
        J = lambda key: want[key]["scalars"][0]
        assert J((0, 1, kind == "disp_lsq", 1, 0)) > 0
        shared = 2 if kind == "disp_lsq" else 1
        assert J((0, 1, kind == "disp_lsq", 1, 0)) == J((shared, 0, kind == "disp_lsq", 1, 0))
        for i in (3, 6):
            assert J((0, 1, kind == "disp_lsq", 1, i)) != J((shared, 0, kind == "disp_lsq", 1, i)), i
            table, row = want[0, 1, kind == "disp_lsq", 1, i], want["row", i]
            assert np.array_equal(table["g"], row["g"]) and np.array_equal(table["pxy"], row["pxy"]), i
            assert table["scalars"][:4].tobytes() == row["scalars"][:4].tobytes(), i  # J and the explicit partials


# ---- refinement ------------------------------------------------------------------------------------------------------------------
REFINED = ("xy", "conn", "u_known", "u_in", "f_in", "node_parents", "elem_parent")


def test_refine_reads_device_marks_and_indicators_and_downloads_every_type(built):
    prob = MESHES["frontal3k"][0]()
    E = prob.mesh.num_elements
    marks = (np.random.default_rng(E).random(E) < 0.1).astype(np.uint8)
    with two_legs() as legs:
        def run(leg):
            c = leg.ctx
            c.solve(prob)
            c.run_stress("run")
            eta2 = written(leg.download_stress("run", 0), "run")["eta2"]  # down into `memory` and up again from it
            out = {"eta2": dict(eta2=eta2)}
            assert leg.run_refine("marks", split=3, marks=marks) == MAG_OK, leg.error()
            out["marks"] = leg.download_refine()
            for rule, theta in (("max_fraction", 0.3), ("top_fraction", 0.2)):
                assert leg.run_refine(rule, theta=theta, indicator=eta2) == MAG_OK, leg.error()
                out[rule] = leg.download_refine()
                c.run_refine(rule=rule, theta=theta)  # indicator = NULL: the same eta2, read where it lies
                out[rule, "held"] = leg.download_refine()
            assert leg.run_refine("marks", marks=np.zeros(E, dtype=np.uint8)) == MAG_OK, leg.error()
            out["no marks"] = leg.download_refine()
            return out
        want, got = in_all_legs(legs, run)
        for key in want:
            if key != "no marks":  # (below: its node_parents are what either leg handed in)
                assert_same_bits(got[key], want[key], key)
        eta2 = want["eta2"]["eta2"]
        twins = {"marks": dict(marks=marks, split=3), "max_fraction": dict(indicator=eta2, rule="max_fraction", theta=0.3),
                 "top_fraction": dict(indicator=eta2, rule="top_fraction", theta=0.2)}
        for key, kw in twins.items():
            twin = refine_ref.of_problem(prob, **kw)
            assert got[key]["marked_edges"] >= 1 and got[key]["nodes"] == twin["nodes"]
            for k in REFINED:
                assert got[key][k].dtype == twin[k].dtype and got[key][k].tobytes() == twin[k].tobytes(), (key, k)
            if key != "marks":
                assert_same_bits(got[key, "held"], got[key], (key, "the held indicator"))
        # no node added: node_parents is not written, on either leg
        for leg, out in zip(legs, (want, got)):
            assert out["no marks"]["marked_edges"] == 0 and out["no marks"]["elements"] == E
            assert (out["no marks"]["node_parents"].view(np.uint8) == UNWRITTEN[leg.memory]).all()
        for k in REFINED:
            if k != "node_parents":
                assert got["no marks"][k].tobytes() == want["no marks"][k].tobytes(), k


# ---- modal analysis --------------------------------------------------------------------------------------------------------------
def test_download_modal_into_device_buffers(built):
    prob = MESHES["plate16"][0]()
    with two_legs() as legs:
        def run(leg):
            leg.ctx.upload_problem(prob)
            leg.ctx.run_modal(modes=3, density=RHO)
            return written(leg.download_modal(), "modal")
        want, got = in_all_legs(legs, run)
        assert_same_bits(got, want, "modal")
        assert want["shapes"].shape == (3, 2 * prob.mesh.num_nodes) and (np.diff(want["lambda"]) > 0).all()
        assert np.array_equal(want["frequency"], np.sqrt(want["lambda"]) / (2.0 * np.pi))
        assert_same_bits(legs[1].ctx.download_modal(), want, "modal to the host")


# ---- the element stiffness field and the design ----------------------------------------------------------------------------------
def design_problem():
    return dref.cantilever(dref.TOPOPT_MESHES["plate_32x16"]())


def test_the_field_and_two_design_iterations_from_device_memory(built):
    prob = design_problem()
    E = prob.mesh.num_elements
    rng = np.random.default_rng(4)
    scale, rho0 = 10.0 ** rng.uniform(-2, 0, E), rng.uniform(0.2, 1.0, E)
    g = prob.f_in.copy()  # J = f^T u, the compliance: dJ/ds < 0 everywhere
    with two_legs() as legs:
        def run(leg):
            c = leg.ctx
            c.upload_problem(prob)
            assert leg.set_element_scale(scale) == MAG_OK, leg.error()
            c.run()
            out = {"field": dict(zip(("u", "f", "stress"), c.download()))}
            assert leg.design_init(rho0, filter_passes=2) == MAG_OK, leg.error()
            out["init"] = written(leg.download_design(), "init")
            out["init", "info"] = c.design_info()
            for k in range(2):
                c.run()
                assert leg.run_adjoint("run", g) == MAG_OK, leg.error()
                delem = leg.download_adjoint("run", 0, want=("delem",))["delem"]  # into `memory`, divided on the host
                s = leg.download_design()["scale"]
                assert leg.design_step(delem / s) == MAG_OK, leg.error()
                out[k] = written(leg.download_design(), k)
                out[k, "info"] = c.design_info()
            c.run()
            out["last"] = dict(zip(("u", "f", "stress"), c.download()))
            return out
        want, got = in_all_legs(legs, run)
        for key in want:
            assert_same_bits(got[key], want[key], key)
        assert_same_bits(legs[1].ctx.download_design(), want[1], "the design to the host")
        assert want[1, "info"]["steps"] == 2 and want[1, "info"]["change"] > 0 and np.abs(want[1]["dJ_drho"]).max() > 0
        assert not np.array_equal(want[0]["rho"], want[1]["rho"]) and np.array_equal(want["init"]["rho"], rho0)


# ---- bad values that live on the device ------------------------------------------------------------------------------------------
def refused_alike(legs, call, needle):
    """the same status and the same text on both legs; `needle` names the offender"""
    (rc_h, msg_h), (rc_d, msg_d) = in_all_legs(legs, lambda leg: (call(leg), leg.error()))
    assert rc_h == rc_d == MAG_ERR_BAD_ARGS, (rc_h, msg_h, rc_d, msg_d)
    assert msg_h == msg_d and needle in msg_d, (msg_h, msg_d)


def test_a_bad_material_on_the_device_is_refused_like_its_host_twin_and_leaves_the_variants(built):
    prob = MESHES["plate16"][0]()
    xy, mat, u, f = make_variants(prob, 4, seed=11)
    bad = mat.copy()
    bad[2, 1] = -1.0  # poisson_ratio^2 == 1 in variant 2 of 4
    with two_legs() as legs:
        def before(leg):
            leg.ctx.upload_problem(prob)
            assert leg.set_variants(4, xy, mat, u, f) == MAG_OK, leg.error()
            leg.ctx.run_variants()
            leg.ctx.run_sensitivities("variants")
            return leg.download_variant(1), leg.download_sensitivity("variants", 1)
        kept = in_all_legs(legs, before)
        for given in (dict(xy=xy, material=bad, u_in=u, f_in=f), dict(material=bad)):
            refused_alike(legs, lambda leg: leg.set_variants(4, **given), "variant 2: poisson_ratio^2 == 1")
            # a refused material leaves the set, its results and what was derived from them as they were, on both legs
            after = in_all_legs(legs, lambda leg: (leg.download_variant(1), leg.download_sensitivity("variants", 1)))
            for a, b in zip(after, kept):
                assert_same_bits(a[0], b[0], "the variants stay")
                assert_same_bits(a[1], b[1], "their sensitivities stay")
        assert_same_bits(kept[1][0], kept[0][0], "before")

        def again(leg):  # the context still works
            assert leg.set_variants(4, material=mat[::-1]) == MAG_OK, leg.error()
            leg.ctx.run_variants()
            return leg.download_variant(3)
        want, got = in_all_legs(legs, again)
        assert_same_bits(got, want, "after the refusal")


def test_a_bad_scale_on_the_device_is_refused_and_the_field_stays(built):
    prob = design_problem()
    E = prob.mesh.num_elements
    scale = 10.0 ** np.random.default_rng(4).uniform(-2, 0, E)
    with two_legs() as legs:
        def before(leg):
            leg.ctx.upload_problem(prob)
            assert leg.set_element_scale(scale) == MAG_OK, leg.error()
            leg.ctx.run()
            return dict(zip(("u", "f", "stress"), leg.ctx.download()))
        want, got = in_all_legs(legs, before)
        assert_same_bits(got, want, "under the field")
        for value in (0.0, np.nan):
            bad = scale.copy()
            bad[[E // 3, E // 2]] = value
            refused_alike(legs, lambda leg: leg.set_element_scale(bad), f"scale[{E // 3}]")
            for leg in legs:  # the field as it was: the results stand, and a new run gives them again
                assert_same_bits(dict(zip(("u", "f", "stress"), leg.ctx.download())), want, ("results kept", value))
                leg.ctx.run()
                assert_same_bits(dict(zip(("u", "f", "stress"), leg.ctx.download())), want, ("re-run", value))
                assert leg.ctx.stats()["cg_kernel"] == 3


def test_a_bad_rho0_on_the_device_is_refused_like_its_host_twin(built):
    prob = design_problem()
    E = prob.mesh.num_elements
    rho0 = np.random.default_rng(4).uniform(0.2, 1.0, E)
    with two_legs() as legs:
        for leg in legs:
            leg.ctx.upload_problem(prob)
        for value in (0.0, 1.0 + 2.0 ** -52, -0.5, np.nan):
            bad = rho0.copy()
            bad[[E // 3, E // 2]] = value
            refused_alike(legs, lambda leg: leg.design_init(bad), f"rho0[{E // 3}] is outside (0, 1]")

        def again(leg):
            assert leg.design_init(rho0) == MAG_OK, leg.error()
            leg.ctx.run()
            return dict(leg.download_design(), u=leg.ctx.download()[0])
        want, got = in_all_legs(legs, again)
        assert_same_bits(got, want, "after the refusals")


def test_a_bad_indicator_on_the_device_is_refused_with_the_offender_and_its_value(built):
    prob = MESHES["plate16"][0]()
    E = prob.mesh.num_elements
    ind = np.random.default_rng(E).random(E)
    with two_legs() as legs:
        for leg in legs:
            leg.ctx.upload_problem(prob)
        for value, text in ((np.nan, "nan"), (-0.25, "-0.25")):
            bad = ind.copy()
            bad[[17, 90]] = value
            for rule in ("top_fraction", "max_fraction"):
                refused_alike(legs, lambda leg: leg.run_refine(rule, indicator=bad), f"indicator[17] = {text} is not finite and >= 0")

        def again(leg):
            assert leg.run_refine("top_fraction", theta=0.2, indicator=ind) == MAG_OK, leg.error()
            return leg.download_refine()
        want, got = in_all_legs(legs, again)
        assert_same_bits(got, want, "after the refusals")
        twin = refine_ref.of_problem(prob, indicator=ind, rule="top_fraction", theta=0.2)
        for k in REFINED:
            assert got[k].tobytes() == twin[k].tobytes(), k


# ---- transient dynamics ------------------------------------------------------------------------------------------------------------
def test_the_transient_pass_reads_and_writes_device_memory(built):
    """mag_run_transient (amplitude, u0, v0, probes), mag_download_transient (nine arrays and the int32 iterations, which come from
    the host) and mag_assemble_effective: the doubles on an 8-byte boundary that is no 16-byte one, the int32 arrays on a 4-byte
    boundary that is no 8-byte one"""
    import test_transient_gpu as tg
    from test_transient_paths_gpu import some_probes
    prob, K, M, free, w1, T1 = tg.setup("plate16", "load")
    n2 = 2 * prob.mesh.num_nodes
    beta, gamma, alpha, eta = tg.parameters("damped", w1)
    dt = T1 / 200.0
    u0, v0 = transient_ref.moving_start(K, M, free, prob.u_in, prob.f_in, modal_ref.eigenpairs(K, M, free, 4)[1], alpha, eta)
    amp = tg.amplitude_of("load", dt, T1, 15)
    resumed_amp = amp[10:].copy()
    resumed_amp[0] = np.nan  # (ignored)
    probes = some_probes(prob)
    assert len(probes) == 300 and probes.max() == n2 - 1
    opts = dict(beta=beta, gamma=gamma, rayleigh_mass=alpha, rayleigh_stiffness=eta, energies=1, snapshot_every=3, cg_tol=tg.CG_TOL)
    with two_legs(offset=8) as legs:
        def run(leg):
            c = leg.ctx
            c.upload_problem(prob)
            out = {}
            assert leg.run_transient(10, dt, RHO, amp[:11], u0, v0, probes, **opts) == MAG_OK, leg.error()
            out["first"] = written(leg.download_transient(), "first")
            out["first, three members"] = leg.download_transient(want=("v", "probe_a", "iterations"))
            out["first, to the host"] = c.download_transient(num_probes=len(probes), energies=True)
            assert leg.run_transient(5, dt, RHO, resumed_amp, probes=probes[:7], resume=1, **opts) == MAG_OK, leg.error()
            out["resumed"] = written(leg.download_transient(), "resumed")
            out["effective"] = written(dict(values=leg.assemble_effective(0.37, 2.5e4, RHO)), "effective")
            out["resumed, afterwards"] = leg.download_transient()  # (mag_assemble_effective overwrites A, not the results)
            return out
        want, got = in_all_legs(legs, run)
        for key in want:
            assert_same_bits(got[key], want[key], key)
        assert list(got["first, three members"]) == ["v", "probe_a", "iterations", "t_start", "t_end"]
        assert got["first"]["iterations"].dtype == np.int32 and got["first"]["iterations"].min() > 0
        assert got["first"]["probe_u"].shape == (11, 300) and got["first"]["snapshots"].shape == (4, n2) and got["first"]["energies"].shape == (11, 3)
        assert got["resumed"]["probe_u"].shape == (6, 7) and got["resumed"]["snapshots"].shape == (2, n2)
        assert_same_bits(got["resumed, afterwards"], got["resumed"], "after mag_assemble_effective")
        for k in got["first, three members"]:
            assert np.array_equal(got["first, three members"][k], got["first"][k]), k
        for k, a in got["first, to the host"].items():
            assert np.array_equal(a, got["first"][k]), k
        # the binding's own path, host memory throughout, on a third context
        with Context(device=0) as c:
            kw = dict(dt=dt, density=RHO, beta=beta, gamma=gamma, rayleigh=(alpha, eta), energies=True, snapshot_every=3, cg_tol=tg.CG_TOL)
            first = c.transient(prob, steps=10, amplitude=amp[:11], u0=u0, v0=v0, probes=probes, **kw)
            resumed = c.transient(steps=5, amplitude=resumed_amp, probes=probes[:7], resume=True, **kw)
            effective = c.assemble_effective(0.37, 2.5e4, RHO)
        for key, ref in (("first", first), ("resumed", resumed)):
            for k, a in got[key].items():
                assert np.array_equal(a, ref[k]), (key, k)
        assert np.array_equal(got["effective"]["values"], effective)
        # a probe outside [0, 2N) that lives on the device: refused like its host twin, and the earlier results are gone
        bad = probes[:9].copy()
        bad[5] = n2
        refused_alike(legs, lambda leg: leg.run_transient(4, dt, RHO, probes=bad, **opts), "probes[5]")
        for leg in legs:
            with pytest.raises(MagnetiteError) as e:
                leg.ctx.download_transient()
            assert e.value.code == 7  # MAG_ERR_STATE
