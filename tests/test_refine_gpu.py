"""GPU: mag_run_refine against its numpy twin (tests/refine_ref.py) -- every array of the refined mesh exactly, for every rule,
both splits, two sets of boundary data; a repeat gives the same bits; nothing else of the context changes; mag_upload_refined is
the host round trip bit for bit; the refined mesh solves to the oracle's answer; and the adaptive loop refines where the twin
does, with a relative error estimate that falls every round."""
import functools

import numpy as np
import pytest

import refine_ref as ref
from magnetite_amd import Context, meshgen
from magnetite_amd.meshgen import Mesh, Problem

pytestmark = pytest.mark.gpu

ARRAYS = ("xy", "conn", "u_known", "u_in", "f_in", "node_parents", "elem_parent")
WORDS = ("nodes", "elements", "marked", "marked_edges", "split2", "split3", "split4")
CONFIGS = {"pull": meshgen.config_fixed_left_pull_right, "point": meshgen.config_fixed_left_point_load}

MESHES = {
    "plate8": lambda: meshgen.plate(8),
    "tie_strip64": lambda: ref.tie_strip(64),
    "frontal24": lambda: meshgen.frontal_like(24),
    "frontal12_clockwise": lambda: meshgen.clockwise(meshgen.frontal_like(12)),
    "holes24_shuffled": lambda: meshgen.shuffle(meshgen.plate_with_holes(24), 7),
    "plate96": lambda: meshgen.plate(96),  # 18k elements: the sorts and scans cross their block boundaries
}
SOLVABLE = ("plate8", "frontal24", "holes24_shuffled", "plate96")  # counter-clockwise: K is positive definite


@functools.lru_cache(maxsize=None)
def problem(name, config):
    return CONFIGS[config](MESHES[name]())


def assert_equals_twin(got, want, what):
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    for k in WORDS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["sweeps"] == want["sweeps"], (what, got["sweeps"], want["sweeps"])  # (a sweep reads the flags from before it)


def some_marks(name, E):
    if name == "tie_strip64":
        rows = np.zeros((3, E), dtype=np.uint8)
        rows[0, 0] = rows[1, E // 2] = rows[2, E - 1] = 1  # the last one: a closure through the whole strip
        return list(rows)
    rng = np.random.default_rng(E)
    return [(rng.random(E) < 0.1).astype(np.uint8), (np.arange(E) == E // 3).astype(np.uint8)]


def an_indicator(E):
    """Equal values (ties at the cut of either rule), zeros and a -0.0."""
    rng = np.random.default_rng(E + 1)
    ind = np.round(rng.random(E) * 8) / 8 + np.where(rng.random(E) < 0.3, rng.random(E), 0.0)
    ind[E // 2] = -0.0
    ind[E // 5] = 0.0
    return ind


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(MESHES))
def test_every_array_equals_the_twins(built, name, config):
    prob = problem(name, config)
    E = prob.mesh.num_elements
    ind = an_indicator(E)
    with Context(device=0) as c:
        c.upload_problem(prob)
        for split in (1, 3):
            for i, marks in enumerate(some_marks(name, E)):
                got = c.refine(marks=marks, split=split)
                want = ref.of_problem(prob, marks=marks, split=split)
                print(name, config, "marks", i, "split", split, {k: got[k] for k in WORDS}, "sweeps", got["sweeps"], "twin", want["sweeps"])
                assert_equals_twin(got, want, ("marks", i, split))
            for rule, theta in (("max_fraction", 0.5), ("max_fraction", 1.0), ("top_fraction", 0.2), ("top_fraction", 1e-9), ("top_fraction", 1.0)):
                got = c.refine(indicator=ind, rule=rule, theta=theta, split=split)
                want = ref.of_problem(prob, indicator=ind, rule=rule, theta=theta, split=split)
                print(name, config, rule, theta, "split", split, {k: got[k] for k in WORDS}, "sweeps", got["sweeps"], "twin", want["sweeps"])
                assert_equals_twin(got, want, (rule, theta, split))
            got = c.refine(indicator=np.zeros(E), rule="max_fraction", theta=0.5, split=split)
            assert got["marked"] == 0 and got["elements"] == E  # nothing is marked when the maximum is 0
            assert_equals_twin(got, ref.of_problem(prob, indicator=np.zeros(E), rule="max_fraction", theta=0.5, split=split), ("zero", split))


@pytest.mark.parametrize("name", SOLVABLE)
def test_the_devices_own_indicator(built, name):
    """indicator = None: the eta2 of run_stress("run"), read where it lies; the twin is given the downloaded eta2."""
    prob = problem(name, "pull")
    with Context(device=0) as c:
        c.solve(prob)
        eta2 = c.stress_recovery("run")[0]["eta2"]
        for split in (1, 3):
            for rule, theta in (("top_fraction", 0.2), ("max_fraction", 0.3)):
                got = c.refine(rule=rule, theta=theta, split=split)
                want = ref.of_problem(prob, indicator=eta2, rule=rule, theta=theta, split=split)
                print(name, rule, theta, "split", split, {k: got[k] for k in WORDS}, "sweeps", got["sweeps"], "twin", want["sweeps"])
                assert got["marked"] >= 1
                assert_equals_twin(got, want, (rule, split))


def test_a_bad_indicator_is_refused_with_the_first_offender_named(built):
    from magnetite_amd.solver import MagnetiteError
    prob = problem("plate8", "pull")
    E = prob.mesh.num_elements
    with Context(device=0) as c:
        c.upload_problem(prob)
        with pytest.raises(MagnetiteError) as e:  # no recovery held
            c.run_refine(rule="top_fraction")
        assert e.value.code == 7
        for bad in (np.nan, np.inf, -1e-300):
            ind = np.ones(E)
            ind[[17, 90]] = bad
            for rule in ("top_fraction", "max_fraction"):
                with pytest.raises(MagnetiteError) as e:
                    c.run_refine(indicator=ind, rule=rule)
                assert e.value.code == 1 and "indicator[17]" in str(e.value), str(e.value)
                with pytest.raises(MagnetiteError):
                    c.refine_info()  # a refused call holds no refinement


def test_a_repeat_gives_the_same_bits(built):
    prob = problem("holes24_shuffled", "point")
    marks = some_marks("holes24_shuffled", prob.mesh.num_elements)[0]
    with Context(device=0) as c:
        c.upload_problem(prob)
        first = c.refine(marks=marks, split=3)
        other = c.refine(marks=1 - marks, split=1)
        again = c.refine(marks=marks, split=3)
    assert other["elements"] != first["elements"]
    for k in ARRAYS:
        assert first[k].tobytes() == again[k].tobytes(), k
    assert {k: first[k] for k in WORDS} == {k: again[k] for k in WORDS}


def test_nothing_else_of_the_context_changes(built):
    prob = problem("frontal24", "pull")
    with Context(device=0) as c:
        c.solve(prob)
        c.run_stress("run")
        c.run_sensitivities("run")
        before = (c.download(), c.stats(), c.download_stress("run", 0), c.download_sensitivity("run", 0))
        c.refine(rule="top_fraction", theta=0.2)
        c.refine(marks=np.ones(prob.mesh.num_elements, dtype=np.uint8), split=3)
        after = (c.download(), c.stats(), c.download_stress("run", 0), c.download_sensitivity("run", 0))
        fresh = (c.stress_recovery("run")[0], c.sensitivities("run")[0])
    for a, b in zip(before[0], after[0]):
        assert a.tobytes() == b.tobytes()
    assert before[1] == after[1]
    for a, b in ((before[2], after[2]), (before[3], after[3]), (before[2], fresh[0]), (before[3], fresh[1])):
        assert a.keys() == b.keys()
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("split", [1, 3])
def test_upload_refined_is_the_host_round_trip(built, split):
    prob = problem("holes24_shuffled", "pull")
    with Context(device=0) as c, Context(device=0) as d:
        c.solve(prob)
        c.stress_recovery("run")
        c.run_refine(rule="top_fraction", theta=0.2, split=split)
        m = c.download_refine()
        c.upload_refined()
        assert (c.N, c.E) == (len(m["xy"]), len(m["conn"]))
        c.run()
        on_device = c.download(), c.stats()
        # the refinement's arrays stay readable; the runs of the coarse mesh are gone with the upload
        again = c.download_refine()
        for k in ARRAYS:
            assert again[k].tobytes() == m[k].tobytes(), k
        d.upload(m["xy"], m["conn"], m["u_known"], m["u_in"], m["f_in"], prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
        d.run()
        by_host = d.download(), d.stats()
    for a, b, what in zip(on_device[0], by_host[0], ("u", "f", "stress")):
        assert a.tobytes() == b.tobytes(), what
    for k in ("iterations", "converged", "n_free", "cg_kernel", "final_cost"):
        assert on_device[1][k] == by_host[1][k], k
    assert on_device[1]["converged"] == 1


def test_a_callers_upload_drops_the_refinement(built):
    from magnetite_amd.solver import MagnetiteError
    prob = problem("plate8", "pull")
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.run_refine(marks=np.ones(prob.mesh.num_elements, dtype=np.uint8))
        c.upload_problem(prob)
        for call in (c.refine_info, c.download_refine, c.upload_refined):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == 7


def test_the_refined_mesh_solves_to_the_oracles_answer(built):
    import oracle
    prob = meshgen.config_fixed_left_pull_right(meshgen.plate_with_holes(24))
    with Context(device=0) as c:
        c.solve(prob)
        c.stress_recovery("run")
        c.run_refine(rule="top_fraction", theta=0.2)
        m = c.download_refine()
        c.upload_refined()
        c.run()
        u, _, _ = c.download()
        st = c.stats()
    assert len(m["conn"]) > prob.mesh.num_elements and st["converged"] == 1
    sol = oracle.run(m["xy"].reshape(-1), m["conn"].reshape(-1), m["u_known"], m["u_in"], m["f_in"], prob.youngs_modulus, prob.poisson_ratio,
                     prob.part_thickness, path="sparse")
    err = np.linalg.norm(u - sol["u"]) / np.linalg.norm(sol["u"])
    print("refined holes24: N", len(m["xy"]), "E", len(m["conn"]), "iterations", st["iterations"], "rel-L2(u)", err)
    assert err <= 1e-8


ADAPT_MESHES = {"holes16": lambda: meshgen.plate_with_holes(16), "frontal16": lambda: meshgen.frontal_like(16)}


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("name", list(ADAPT_MESHES))
def test_the_adaptive_loop(built, name, split):
    """Context.adapt over three rounds against the same loop driven by hand, whose every refinement is compared with the twin
    given that round's downloaded eta2: the same meshes, growing every round, with an eta_rel that falls every round (by 10-35 %
    per round on these meshes in float64 on the host: round-off in eta2 at the cut cannot turn that)."""
    prob = meshgen.config_fixed_left_pull_right(ADAPT_MESHES[name]())
    with Context(device=0) as c:
        out = c.adapt(prob, rounds=3, theta=0.2, rule="top_fraction", split=split)
    history = out["history"]
    print(name, "split", split, [(h["nodes"], h["elements"], h["eta_rel"], h["iterations"]) for h in history])
    assert len(history) == 4
    cur, by_hand = prob, []
    with Context(device=0) as c:
        c.upload_problem(cur)
        for r in range(4):
            c.run()
            field = c.stress_recovery("run")[0]
            by_hand.append(dict(nodes=c.N, elements=c.E, eta=field["eta"], eta_rel=field["eta_rel"], iterations=c.stats()["iterations"]))
            if r == 3:
                break
            got = c.refine(rule="top_fraction", theta=0.2, split=split)
            want = ref.of_problem(cur, indicator=field["eta2"], rule="top_fraction", theta=0.2, split=split)
            assert_equals_twin(got, want, (name, split, "round", r))
            c.upload_refined()
            cur = Problem(Mesh(got["xy"], got["conn"]), got["u_known"], got["u_in"], got["f_in"], prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness)
        last = c.download()
    assert history == by_hand
    final = out["problem"]
    assert final.mesh.xy.tobytes() == cur.mesh.xy.tobytes() and final.mesh.conn.tobytes() == cur.mesh.conn.tobytes()
    assert final.u_known.tobytes() == cur.u_known.tobytes() and final.u_in.tobytes() == cur.u_in.tobytes() and final.f_in.tobytes() == cur.f_in.tobytes()
    assert out["result"]["u"].tobytes() == last[0].tobytes() and out["result"]["stress"].tobytes() == last[2].tobytes()
    assert out["recovery"]["eta_rel"] == history[-1]["eta_rel"] and out["result"]["converged"] == 1
    for a, b in zip(history, history[1:]):
        assert b["elements"] > a["elements"] and b["nodes"] > a["nodes"]
        assert b["eta_rel"] < a["eta_rel"], (a, b)


def test_adapt_stops_at_its_target(built):
    prob = meshgen.config_fixed_left_pull_right(meshgen.plate_with_holes(16))
    with Context(device=0) as c:
        full = c.adapt(prob, rounds=2)
        target = full["history"][1]["eta_rel"]
        out = c.adapt(prob, rounds=5, target_eta_rel=target)
        none = c.adapt(prob, rounds=0)
    assert len(out["history"]) == 2 and out["history"] == full["history"][:2]
    assert out["problem"].mesh.num_elements == full["history"][1]["elements"]
    assert len(none["history"]) == 1 and none["problem"] is prob
