"""The numpy twin of mag_run_transient_tl (tests/transient_tl_ref.py) against what is known without a device: the linear Newmark
twin for a small load, the size of the nonlinearity, the order of the scheme, and the admission of the GPU tests' cases
(tests/transient_tl_cases.py) -- the twin's own round-off floor against the GPU bars, every step's residual ratios away from the
threshold that decides an iteration count; and the same admission, with the step at the cap and the definiteness of every matrix
factored, of the cases of tests/test_transient_tl_paths_gpu.py (EARLY, LONG, INVERTED, NEWMARK)."""
import numpy as np
import pytest

import transient_ref
import transient_tl_cases as cases
import transient_tl_ref as ref

TOL = cases.NEWTON_TOL


def run(name, kind, steps, dt, scale=1.0, **kw):
    s = cases.setup(name, kind, nominal=True)
    p = s["prob"]
    return ref.newmark_tl(*ref.of_problem(p), s["M"], s["free"], p.u_in, scale * np.asarray(p.f_in), steps, dt, alpha=s["alpha"], u0=s["u0"],
                          newton_tol=TOL, **kw)


def test_a_small_load_gives_the_linear_newmark_run():
    """f_in scaled by 1e-6: two iterations a step, and the linear twin's run to 1e-5 (measured: 1.7e-7)"""
    s = cases.setup("plate16", "load300", nominal=True)
    p = s["prob"]
    got = run("plate16", "load300", s["steps"], s["dt"], scale=1e-6)
    lin = transient_ref.newmark(s["K"], s["M"], s["free"], p.u_in, 1e-6 * np.asarray(p.f_in), s["steps"], s["dt"])
    err = max(cases.rel(got[k], lin[k]) for k in ("u", "v", "a"))
    print(f"small load: newton {got['newton_iterations'].tolist()} rel {err:.3e}")
    assert got["converged"] and got["newton_iterations"][1:].max() <= 2
    assert err <= 1e-5
    assert cases.rel(got["f"], lin["f"]) <= 1e-5 and cases.rel(got["energies"], lin["energies"]) <= 1e-5


@pytest.mark.parametrize("name,kind", [("beam", "beam"), ("plate16", "load300")])
def test_the_cases_are_nonlinear(name, kind):
    """at the nominal step the run is more than 1e-2 from the linear twin's (measured: 0.13 to 0.18)"""
    s = cases.setup(name, kind, nominal=True)
    p = s["prob"]
    got = run(name, kind, s["steps"], s["dt"])
    lin = transient_ref.newmark(s["K"], s["M"], s["free"], p.u_in, p.f_in, s["steps"], s["dt"])
    d = cases.rel(got["u"][-1], lin["u"][-1])
    print(f"{name} {kind}: rel(u, linear) {d:.3e} min det F {got['min_det']:.3f}")
    assert got["converged"] and d > 1e-2


def test_halving_the_step_quarters_the_error():
    """the average-acceleration scheme is of second order: against a 16 times finer run, half the step has a third to a fifth of the
    error (exactly second order gives 4.05).  The load comes on as 1/2 (1 - cos(pi t / T)) over the T = 0.8 T1 of the run, in 8
    steps: under the cases' step load the high modes of the point load decide the error at any step that can be afforded here
    (measured: ratios of 1.5 to 1.7), and no order shows."""
    s = cases.setup("plate16", "load300", nominal=True)
    n, dt = 8, s["T1"] / 10

    def final(k):
        t = (dt / k) * np.arange(k * n + 1)
        return run("plate16", "load300", k * n, dt / k, amplitude=0.5 * (1.0 - np.cos(np.pi * t / (n * dt))))["u"][-1]

    fine = final(16)
    e1, e2 = cases.rel(final(1), fine), cases.rel(final(2), fine)
    print(f"error at dt {e1:.3e}, at dt / 2 {e2:.3e}: ratio {e1 / e2:.2f}")
    assert 3.0 <= e1 / e2 <= 5.0


def test_the_other_first_iterates_fail_where_the_pass_converges():
    """a' = a_n and a' = 0 at T1 / 20 on the beam: no convergence within 25 iterations, or far more than u' = u_n needs"""
    s = cases.setup("beam", "beam", nominal=True)
    dt = s["T1"] / 20
    good = run("beam", "beam", 4, dt)
    assert good["converged"] and good["newton_iterations"][1:].max() <= 6
    for start in ("a", "0"):
        bad = run("beam", "beam", 4, dt, start=start)
        worst = bad["newton_iterations"][1:].max() if bad["converged"] else None
        print(f"start {start!r}: converged {bad['converged']} steps {bad['steps_done']} most {worst}")
        assert not bad["converged"] or worst > 2 * good["newton_iterations"][1:].max()


def test_the_cap_ends_the_run_at_the_last_converged_step():
    got = run("beam", "beam", 4, cases.setup("beam", "beam").get("dt"), max_newton=2)
    assert not got["converged"] and got["steps_done"] == 0 and got["u"].shape[0] == 1 and len(got["residuals"]) == 2


@pytest.mark.parametrize("name,kind", cases.CASES)
def test_admission_the_twin_is_at_its_floor(name, kind):
    """the twin at newton_tol = 1e-10 is within a tenth of the GPU bars (u 1e-8; v, a, f, energies 1e-7) of its run on to the
    round-off floor (extra = 3).  Measured on plate16: u 4e-12, v 1e-11, a 2e-11."""
    got, floor = cases.twin(name, kind), cases.twin(name, kind, extra=3)
    assert got["converged"] and floor["converged"]
    err = {k: max(cases.rel(got[k][n], floor[k][n]) for n in range(1, len(got[k]))) for k in ("u", "v", "a", "f", "energies")}
    print(f"{name} {kind}: " + " ".join(f"{k} {v:.1e}" for k, v in err.items()))
    assert err["u"] <= 1e-9
    assert max(err[k] for k in ("v", "a", "f", "energies")) <= 1e-8


def off_the_threshold(what, got):
    """the admission rule on the converged steps of a run; returns the ratios past them (those of a step that hit the cap)"""
    its, res = got["newton_iterations"], got["residuals"]
    assert its[0] == 0 and len(its) == got["steps_done"] + 1 and its[1:].sum() <= len(res)
    end = np.cumsum(its[1:])
    last = res[end - 1]
    before = np.array([res[e - 2] if n > 1 else np.inf for n, e in zip(its[1:], end)])
    print(f"{what}: newton {its.tolist()} last max {last.max():.2e} last-but-one min {before.min():.2e}")
    assert last.max() <= TOL / 10
    assert before.min() >= 10 * TOL
    return res[its[1:].sum():]


@pytest.mark.parametrize("name,kind", cases.CASES)
def test_admission_every_step_is_off_the_threshold(name, kind):
    """every step's last residual ratio is at most newton_tol / 10 and its last-but-one at least 10 newton_tol: the device's
    iteration counts are the twin's.  A case that misses this gets another dt (transient_tl_cases.FACTOR), not another test."""
    got = cases.twin(name, kind)
    assert got["converged"]
    assert len(off_the_threshold(f"{name} {kind}", got)) == 0


# ---- the admission of the cases of tests/test_transient_tl_paths_gpu.py: the same rule, change the case and not the test
def at_the_floor(what, got, floor):
    rows = len(got["u"])
    err = {k: max([cases.rel(got[k][n], floor[k][n]) for n in range(1, rows)], default=0.0) for k in ("u", "v", "a", "f", "energies")}
    print(f"{what}: against the floor run " + " ".join(f"{k} {v:.1e}" for k, v in err.items()))
    assert err["u"] <= 1e-9
    assert max(err[k] for k in ("v", "a", "f", "energies")) <= 1e-8


@pytest.mark.parametrize("which", ["EARLY", "LONG", "INVERTED"])
def test_admission_of_the_early_ends(which):
    """plate16 / load300 under the amplitude jump: the converged steps off the threshold, the step at the cap at least 100
    newton_tol, every matrix factored positive definite (ratio > 1e-8), the twin at its floor.  Measured: EARLY 3 steps (5, 4, 4),
    9.0e-6 at the cap; LONG all 8; INVERTED 3 steps, 0.21 at the cap, smallest det F -4.7; definite ratios >= 2.9e-4."""
    kw = getattr(cases, which)
    got = cases.twin_with("plate16", "load300", definite=True, **kw)
    past = off_the_threshold(which, got)
    print(f"{which}: steps done {got['steps_done']} the ratios of the step at the cap {past} smallest det F {got['min_det']:.3f} "
          f"definite {got['definite']:.2e}")
    assert got["definite"] > 1e-8
    if which == "LONG":
        assert got["converged"] and len(past) == 0 and not got["inverted"]
        assert got["newton_iterations"].max() == kw["max_newton"]  # (so that one iteration fewer ends the run early)
    else:
        assert not got["converged"] and got["steps_done"] == cases.JUMP_AT - 1 and len(past) == kw["max_newton"]
        assert past[-1] >= 100 * TOL
        assert got["inverted"] == (which == "INVERTED") and abs(got["min_det"]) >= 1e-3
    done = got["steps_done"]
    at_the_floor(which, got, cases.twin_with("plate16", "load300", extra=3, steps=done, **{**kw, "max_newton": 0}))


@pytest.mark.parametrize("name,kind,beta,gamma,lumped", cases.NEWMARK)
def test_admission_of_the_newmark_parameters(name, kind, beta, gamma, lumped):
    """other (beta, gamma): off the threshold, at the floor, positive definite, and more than 1e-4 from the (1/4, 1/2) run"""
    kw = dict(beta=beta, gamma=gamma, lumped=lumped)
    got = cases.twin_with(name, kind, definite=True, **kw)
    assert got["converged"] and not got["inverted"]
    assert len(off_the_threshold(f"{name} {kind} {kw}", got)) == 0
    at_the_floor(f"{name} {kind} {kw}", got, cases.twin_with(name, kind, extra=3, **kw))
    apart = cases.rel(got["u"][-1], cases.twin(name, kind, lumped=lumped)["u"][-1])
    print(f"{name} {kind} {kw}: definite {got['definite']:.2e} rel(u, the (1/4, 1/2) run) {apart:.2e}")
    assert got["definite"] > 1e-8 and apart > 1e-3
