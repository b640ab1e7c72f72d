"""CPU: the numpy twin of the nonlinear-statics pass (tests/newton_ref.py) on its own -- the tangent against the project's K, its
symmetry, a central difference of the internal force, a rigid motion, and the convergence of the Newton loop on the cases the GPU
tests hold the device against.  Figures measured here: tangent(0) - K exactly 0; symmetry 0; the central difference 6e-12
(plate16), 1.3e-10 (beam); the beam in 8 increments 4 iterations each, smallest det F 0.9575; load300 in 2 increments 4-5 and 4;
pull5 in 1 increment 4 with the predictor, 6-12 when the supports jump first.  At the end: the admission of newton_ref.PATHS, the
cases of tests/test_newton_paths_gpu.py (every integer the device is asked for is off its threshold; figures beside the cases)."""
import numpy as np
import pytest

import explicit_tl_cases as cases
import explicit_tl_ref as tl
import modal_ref
import newton_ref as nr

TOL = 1e-10


def test_the_tangent_at_zero_is_k_and_symmetric():
    for name, kind in (("beam", "beam"), ("plate16", "load300"), ("two_fans", "pull5")):
        p = nr.case_problem(name, kind)
        K = modal_ref.matrices(p, cases.RHO, True)[0]
        KT = nr.tangent(*nr.of_problem(p), np.zeros(2 * p.mesh.num_nodes))
        big = abs(K).max()
        print(name, "tangent(0) - K", abs(KT - K).max() / big, "asymmetry", abs(KT - KT.T).max() / big)
        assert abs(KT - K).max() <= 1e-14 * big
        assert abs(KT - KT.T).max() <= 1e-15 * big


@pytest.mark.parametrize("name, kind, increments", [("plate16", "load300", 2), ("beam", "beam", 8)])
def test_the_tangent_is_the_derivative_of_the_force(name, kind, increments):
    p = nr.case_problem(name, kind)
    a = nr.of_problem(p)
    u = nr.case_run(name, kind, increments)["u"]
    KT = nr.tangent(*a, u)
    assert abs(KT - KT.T).max() <= 1e-15 * abs(KT).max()
    L = np.ptp(p.mesh.xy[:, 0])
    rng = np.random.default_rng(5)
    for _ in range(3):
        d = rng.uniform(-1.0, 1.0, u.size)
        eps = 1e-6 * L
        fd = (tl.tl_force(*a, u + eps * d)[0] - tl.tl_force(*a, u - eps * d)[0]) / (2.0 * eps)
        err = np.linalg.norm(fd - KT @ d) / np.linalg.norm(KT @ d)
        print(name, "central difference against K_T d", err)
        assert err <= 1e-8


def test_an_infinitesimal_rotation_of_a_rotated_part_is_in_the_null_space():
    p = nr.case_problem("plate16", "load300")
    u = cases.rigid_motion(p)
    KT = nr.tangent(*nr.of_problem(p), u)
    x = p.mesh.xy + u.reshape(-1, 2)  # the rotated part; its centre is the centroid moved by (0.3, -0.2)
    c = x.mean(axis=0)
    w = np.stack([-(x[:, 1] - c[1]), x[:, 0] - c[0]], axis=1).reshape(-1)
    got = np.linalg.norm(KT @ w) / (abs(KT).max() * np.linalg.norm(w))
    print("|K_T w| / (|K_T| |w|) at the rigid motion", got)
    assert got <= 1e-10
    assert np.linalg.norm(nr.tangent(*nr.of_problem(p), 0 * u) @ w) > 1e-3 * abs(KT).max() * np.linalg.norm(w)  # (K alone is not blind to it)


def margins(out):
    """every increment's last-but-one ratio >= 100 tol or its last <= tol / 5: a device count that differs is a real finding"""
    at = 0
    for n in out["newton_iterations"][1:]:
        r = out["residuals"][at:at + n]
        assert r[-1] <= TOL
        assert (n == 1 or r[-2] >= 100 * TOL) or r[-1] <= TOL / 5, r
        at += n


def test_the_beam_converges_as_measured():
    p = nr.case_problem("beam", "beam")
    out = nr.case_run("beam", "beam", 8)
    tip = np.flatnonzero(p.mesh.xy[:, 0] > p.mesh.xy[:, 0].max() - 1e-9)
    print("beam: iterations", out["newton_iterations"], "tip u", out["u"].reshape(-1, 2)[tip], "min det F", out["min_det"])
    assert out["converged"] and out["halvings"] == 0
    assert all(abs(n - 4) <= 1 for n in out["newton_iterations"][1:])
    assert abs(out["min_det"] - 0.9575) <= 1e-3
    assert np.allclose(out["load"], np.arange(9) / 8)
    mid = out["u"].reshape(-1, 2)[tip].mean(axis=0)
    assert 0.25 <= -mid[1] <= 0.29 and mid[0] < -0.03  # (the tip comes down a quarter of the length and in by a few percent)
    margins(out)


@pytest.mark.parametrize("increments", [1, 4])
def test_the_line_search_reaches_the_same_equilibrium(increments):
    want = nr.case_run("beam", "beam", 8)["u"]
    out = nr.case_run("beam", "beam", increments, line_search=10)
    err = np.linalg.norm(out["u"] - want) / np.linalg.norm(want)
    print("beam,", increments, "increments with line search: iterations", out["newton_iterations"], "halvings", out["halvings"], "u apart", err)
    assert out["converged"] and out["halvings"] > 0 and err <= 1e-8


@pytest.mark.parametrize("name", cases.FOUR)
def test_load300_and_pull5_converge_as_measured(name):
    load = nr.case_run(name, "load300", 2)
    pull = nr.case_run(name, "pull5", 1)
    print(name, "load300", load["newton_iterations"], "pull5", pull["newton_iterations"])
    assert load["converged"] and pull["converged"]
    assert all(3 <= n <= 6 for n in load["newton_iterations"][1:])
    assert abs(pull["newton_iterations"][1] - 4) <= 1
    margins(load)
    margins(pull)


def test_the_predictor_saves_iterations():
    p = nr.case_problem("frontal3k", "pull5")
    jump = nr.newton(*nr.of_problem(p), p.u_known, p.u_in, p.f_in, increments=1, predictor=False)
    with_it = nr.case_run("frontal3k", "pull5", 1)
    print("frontal3k pull5: predictor", with_it["newton_iterations"][1], "jump", jump["newton_iterations"][1])
    assert jump["converged"] and jump["newton_iterations"][1] >= with_it["newton_iterations"][1] + 2
    assert np.linalg.norm(jump["u"] - with_it["u"]) <= 1e-8 * np.linalg.norm(with_it["u"])


def test_the_cap_leaves_the_start():
    out = nr.case_run("beam", "beam", 1, max_newton=2)
    assert not out["converged"] and out["converged_increments"] == 0 and not out["u"].any() and len(out["residuals"]) == 2


# ---- the admission of the cases of tests/test_newton_paths_gpu.py (newton_ref.PATHS): change the case, not the test
@pytest.mark.parametrize("key", list(nr.PATHS))
def test_admission_of_the_path_cases(key):
    """Every converged increment's last ratio <= newton_tol / 10 and last-but-one >= 10 newton_tol; an increment at the cap stands
    at >= 100 newton_tol; with a search, every trial has |min det F| >= 1e-3 and, where the energy test is live, is 1e-9 max(|Pi0|,
    W) from its threshold; every tangent factored is positive definite (eigenvalue ratio > 1e-8).  Then the device's integers
    are the twin's."""
    out, opts = nr.path_run(key), nr.path_options(key)
    its, res = out["newton_iterations"], out["residuals"]
    end = np.cumsum(its[1:])
    last = res[end - 1]
    before = np.array([res[e - 2] if n > 1 else np.inf for n, e in zip(its[1:], end)])
    past = res[its[1:].sum():]
    print(f"{key}: newton {its.tolist()} last max {last.max():.2e} last-but-one min {before.min():.2e} past the converged {past} "
          f"definite {out['definite']:.2e} inverted {out['inverted']} halvings {out['halvings']} steps {out['step_lengths'].tolist()}")
    assert last.max() <= TOL / 10 and before.min() >= 10 * TOL
    assert out["definite"] > 1e-8
    if out["converged"]:
        assert len(past) == 0
    else:
        assert len(past) == opts["max_newton"] and past[-1] >= 100 * TOL
    if opts.get("line_search", 0) > 0:
        tr = out["trials"]
        dets = np.array([abs(t[3]) for t in tr])
        # (from the unloaded start Pi0 = W = 0: every energy excess but 0 is infinitely far from the threshold on that scale)
        live = np.array([abs(t[4]) / t[5] if t[5] > 0.0 else (np.inf if t[4] != 0.0 else 0.0)
                         for t in tr if t[6] < 0.0 and abs(t[2] * t[6]) > 1e-13 * t[5]])
        print(f"{key}: trials {len(tr)} smallest |min det F| {dets.min():.3e} live energy tests {len(live)} smallest margin {live.min():.2e}")
        assert dets.min() >= 1e-3
        assert live.min() >= 1e-9


def test_the_path_cases_take_the_paths_they_are_named_for():
    """what each case is there for, on the twin: the early end after two increments; accepted inverted states that end in a sound
    one; halvings that only the inverted trial causes, and only the energy rule; a moving support under a search that never halves"""
    early = nr.path_run("early")
    assert not early["converged"] and early["converged_increments"] == 2 and early["newton_iterations"].tolist() == [0, 4, 4]
    assert len(early["residuals"]) == 12 and early["load"].tolist() == [0.0, 0.125, 0.25]
    through, p = nr.path_run("through"), nr.path_problem("through")
    assert through["converged"] and through["inverted"] and through["halvings"] == 0
    assert min(d for _, d in through["iterates"]) < -1.0 and through["iterates"][-1][1] > 0.1
    assert nr.element_rows(*nr.of_problem(p), through["u"])[:, 6].min() > 0.1
    for key, steps in (("inversion72", [0.25, 1, 1, 1, 1, 1, 1]), ("inversion320", [0.125, 1, 1, 1, 1, 1, 1, 1])):
        out = nr.path_run(key)
        assert out["converged"] and not out["inverted"] and out["step_lengths"].tolist() == steps
        halved = [t for t in out["trials"] if t[1] == 1][:-1]  # (the trials of iteration 1 that were rejected)
        assert len(halved) == out["halvings"] and halved[0][3] <= -1e-3  # (s = 1 is inverted; the energy rule rejects it as well)
    for key, steps in (("energy1", [0.5, 1, 0.5] + [1] * 7), ("energy2", [0.25] + [1] * 9)):
        out = nr.path_run(key)
        assert out["converged"] and out["step_lengths"].tolist() == steps and out["halvings"] == 2
        assert min(t[3] for t in out["trials"]) > 0.9  # (no trial is inverted: the energy rule alone)
    pull = nr.path_run("pull")
    assert pull["converged"] and pull["halvings"] == 0 and (pull["step_lengths"] == 1.0).all() and pull["min_det"] > 0.5
    assert np.abs(nr.path_problem("pull").u_in).max() > 0  # (du_P != 0 in the slope of iteration 1)
    # pull7: every rejected trial is inverted under a slope g >= 0, where the energy test is skipped -- the inverted trial alone
    # decides; and the supports, moved by s < 1 three times, stand at u_in in the end
    pull7, p7 = nr.path_run("pull7"), nr.path_problem("pull7")
    known = np.asarray(p7.u_known).reshape(-1) != 0
    assert pull7["converged"] and not pull7["inverted"] and pull7["halvings"] == 7
    assert pull7["step_lengths"].tolist() == [0.25, 0.125, 0.25, 1, 1, 1, 1]
    trials = pull7["trials"]
    rejected = [t for t, after in zip(trials, trials[1:]) if after[1] == t[1]]
    assert len(rejected) == 7 and all(t[3] <= -1e-3 and t[6] >= 0.0 for t in rejected)
    gap = np.abs(pull7["u"][known] - np.asarray(p7.u_in)[known]).max() / np.abs(p7.u_in).max()
    print("pull7: the supports against u_in", gap)
    assert gap <= 4 * np.finfo(float).eps
