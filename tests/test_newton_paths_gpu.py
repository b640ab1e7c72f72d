"""GPU: the paths of mag_run_newton that tests/test_newton_gpu.py only brushes, on the cases of newton_ref.PATHS (admitted on the
CPU in tests/test_newton.py: every integer asked of the device here is off its threshold on the twin) -- a run that ends early
after converged increments and its continuation, the line search's step lengths (by the energy rule, by an inverted trial, with a
moving support, without the tables, on the CSR operator's phase), `inverted`, device buffers on an early-ended run.

Bars (the project's own, tests/test_newton_gpu.py): integers -- iteration counts, step lengths (powers of two), halvings,
increments done, `inverted` -- equal the twin's; "the same bits" is tobytes() equality of two device runs; rel(u, u*) <= 2 newton_tol
ref / (lambda_min(K_T,FF(u*)) |u*_F|) with u* the twin run three iterations on to its floor; residual ratios above 1e-8 within rel
1e-4 of the twin's.  Every test prints its figures before it asserts.

Measured on an MI355X (NT-paths): the early end -- 2 increments done, newton_iterations [0, 4, 4, 0], 12 residuals within
9.7e-12 of the twin's, increment 3 at 3.555e-03 at the cap, the same bits as the two-increment run, the continuation 3.9e-14 from
u* (bound 1.3e-8); step lengths, halvings, iteration counts and `inverted` equal the twin's in all twelve searched runs, rel(u, u*)
at most 3.0e-14 against bounds of 1.0e-9 to 1.3e-8, the supports exactly at lambda u_in; through inverted states (det F down to
-5.1) 10 iterations, inverted = 1, the returned state's smallest det F 0.77, rel(u, u*) 5.2e-16.

Found by the pull of 7 lx (the only case whose first iteration is shortened while its supports move): the driver ran the support
predictor in iteration 1 alone, so the supports stayed at s lambda u_in -- step lengths [1/4, 1, 1, 1, 1, 1], 6 iterations,
converged = 1 with the right edge at a quarter of u_in, where the header's u_P = lambda u_in needs [1/4, 1/8, 1/4, 1, 1, 1, 1]."""
import numpy as np
import pytest

import newton_ref as nr
from device_buffers import DeviceArena
from magnetite_amd import Context
from magnetite_amd._lib import MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK
from test_load_cases_gpu import rel
from test_newton_gpu import CONTEXTS, TOL, NewtonLeg

pytestmark = pytest.mark.gpu

RECORDS = ("probe_u", "snapshots", "load", "energies", "newton_iterations")  # (one row per increment)
PER_ITERATION = ("residuals", "step_lengths", "cg_iterations")


def known_of(p):
    return np.asarray(p.u_known).reshape(-1) != 0


def within_the_bound(what, p, u, floor):
    """rel(u, u*) against the first-order bound 2 newton_tol ref / (lambda_min |u*_F|)"""
    u_star, lam_min, ref = floor
    bound = 2 * TOL * ref / (lam_min * np.linalg.norm(u_star[~known_of(p)]))
    err = rel(u, u_star)
    print(what, "rel(u, u*)", err, "bound", bound, "lambda_min", lam_min)
    assert err <= bound


# ---- 1. an early end after converged increments
@CONTEXTS
def test_an_early_end_keeps_the_converged_increments_and_nothing_else(built, context):
    p, opts, want = nr.path_problem("early"), nr.path_options("early"), nr.path_run("early")
    n2 = 2 * p.mesh.num_nodes
    kw = dict(probes=np.arange(n2), snapshots=True)
    with Context(device=0, **context) as c:
        c.upload_problem(p)
        out = c.newton(**opts, **kw)
        two = c.newton(increments=2, load_factors=opts["load_factors"][:2], max_newton=opts["max_newton"], **kw)
        rest = c.newton(increments=3, load_factors=[0.5, 0.75, 1.0], u0=out["u"], snapshots=True)
    print(context, "early end:", out["message"], "newton_iterations", out["newton_iterations"], "residuals", out["residuals"],
          "the twin's", want["residuals"])
    assert out["converged"] == 0 and out["increments_converged"] == 2 and out["inverted"] == 0 and out["halvings"] == 0
    assert out["newton_iterations"].tolist() == [0, 4, 4, 0] and out["newton_iterations_total"] == 12
    assert out["load"].tolist() == [0.0, 0.125, 0.25, 0.0]
    assert not out["probe_u"][3].any() and not out["snapshots"][3].any() and not out["energies"][3].any()
    assert len(out["residuals"]) == len(out["step_lengths"]) == len(out["cg_iterations"]) == 12
    assert out["cg_iterations"].sum() == out["cg_iterations_total"] and (out["step_lengths"] == 1.0).all()
    assert "increment 3 " in out["message"] and "4 iterations" in out["message"] and "mag_run_newton" in out["message"]
    assert np.array_equal(want["newton_iterations"], [0, 4, 4]) and len(want["residuals"]) == 12
    early = want["residuals"] > 1e-8
    err = rel(out["residuals"][early], want["residuals"][early])
    print(context, "residual ratios above 1e-8 against the twin's", err)
    assert err <= 1e-4
    assert out["residuals"][-1] > 100 * TOL  # (the increment at the cap stands far from the tolerance)
    # the failed increment leaves no trace: the state, the reactions, the element rows and rows 0..2 are a two-increment run's
    assert two["converged"] == 1 and two["increments_converged"] == 2
    for k in ("u", "f", "elem"):
        assert out[k].tobytes() == two[k].tobytes(), k
    for k in RECORDS:
        assert out[k][:3].tobytes() == two[k].tobytes(), k
    for k in PER_ITERATION:
        assert out[k][:8].tobytes() == two[k].tobytes(), k
    assert np.array_equal(out["probe_u"][2], out["u"]) and np.array_equal(out["snapshots"][2], out["u"])
    known = known_of(p)
    assert np.array_equal(out["f"][~known], (0.25 * np.asarray(p.f_in))[~known])  # (the reactions are under load[done])
    rows = nr.element_rows(*nr.of_problem(p), out["u"])
    e_err = (np.abs(out["elem"] - rows).max(axis=0) / np.abs(rows).max(axis=0)).max()
    f_err = rel(out["f"][known], nr.residual(*nr.of_problem(p), known, p.f_in, 0.25, out["u"])[2][known])
    print(context, "the element rows", e_err, "f_out on P", f_err)
    assert e_err <= 1e-12 and f_err <= 1e-12
    # a continuation from the returned state reaches the beam's equilibrium
    u_star, lam_min = nr.case_floor("beam", "beam", 8)
    ref = nr.residual(*nr.of_problem(p), known, p.f_in, 1.0, u_star)[1]
    assert rest["converged"] == 1 and rest["snapshots"][0].tobytes() == out["u"].tobytes() and rest["load"].tolist() == [0.0, 0.5, 0.75, 1.0]
    within_the_bound(f"{context} continued from the early end:", p, rest["u"], (u_star, lam_min, ref))


# ---- 2. the line search's steps are the twin's
SEARCHES = [(key, {}, 0) for key in ("energy1", "energy2", "inversion72", "inversion320", "pull", "pull7")]
SEARCHES += [(key, dict(op_variant=1), 0) for key in ("energy1", "inversion72", "pull7")]
SEARCHES += [(key, {}, 4) for key in ("energy1", "inversion72", "pull7")]


@pytest.mark.parametrize("key, context, cg", SEARCHES, ids=[f"{k}-{'op_variant1' if c else 'tables'}-cg{g}" for k, c, g in SEARCHES])
def test_the_line_search_takes_the_twins_steps(built, key, context, cg):
    p, opts, want = nr.path_problem(key), nr.path_options(key), nr.path_run(key)
    known = known_of(p)
    with Context(device=0, **context) as c:
        out = c.newton(p, cg=cg, **opts)
    print(key, context, "cg", cg, "step_lengths", out["step_lengths"], "the twin's", want["step_lengths"], "halvings", out["halvings"], want["halvings"],
          "newton_iterations", out["newton_iterations"], want["newton_iterations"], "inverted", out["inverted"], want["inverted"])
    assert out["cg_kernel"] == (3 if context or cg == 4 else 5)
    assert out["step_lengths"].tolist() == want["step_lengths"].tolist()
    assert out["halvings"] == want["halvings"]
    assert np.array_equal(out["newton_iterations"], want["newton_iterations"])
    assert out["converged"] == 1 and out["inverted"] == int(want["inverted"])
    early = want["residuals"] > 1e-8
    err = rel(out["residuals"][early], want["residuals"][early])
    print(key, "residual ratios above 1e-8 against the twin's", err)
    assert err <= 1e-4
    lam = opts.get("load_factors", [1.0])[-1]
    gap = np.abs(out["u"][known] - lam * np.asarray(p.u_in)[known]).max()
    print(key, "the supports against lambda u_in", gap)
    assert gap <= 4 * np.finfo(float).eps * lam * np.abs(p.u_in).max()  # (the last part of the way is u + (lambda u_in - u): two roundings)
    within_the_bound(f"{key} {context} cg {cg}:", p, out["u"], nr.path_floor(key))


def test_a_search_that_never_halves_changes_nothing(built):
    """the pull case with line_search = 6 against line_search = 0: every array has the same bits, and every word but `halvings`
    (which is 0 in both)"""
    p, opts = nr.path_problem("pull"), nr.path_options("pull")
    kw = dict(probes=np.arange(0, 2 * p.mesh.num_nodes, 3), snapshots=True)
    with Context(device=0) as c:
        c.upload_problem(p)
        searched = c.newton(**opts, **kw)
        plain = c.newton(**{**opts, "line_search": 0}, **kw)
    assert list(searched) == list(plain) and searched["halvings"] == 0 and searched["converged"] == 1
    for k in searched:
        if k != "halvings":
            assert np.asarray(searched[k]).tobytes() == np.asarray(plain[k]).tobytes(), k


# ---- 3. inverted
def test_inverted_is_of_the_accepted_states(built):
    """plain Newton through inverted states raises info[6] with no error and ends in a sound state; the search that rejects the
    inverted trial of the same load leaves it at 0; mag_internal_force reports an inverted iterate of the twin's as inverted"""
    p, want = nr.path_problem("through"), nr.path_run("through")
    a = nr.of_problem(p)
    assert want["inverted"] and nr.element_rows(*a, want["u"])[:, 6].min() > 0  # (the twin first)
    worst, det = min(want["iterates"], key=lambda s: s[1])
    assert det < -1.0 and any(t[3] <= 0.0 for t in nr.path_run("inversion72")["trials"])
    with Context(device=0) as c:
        c.upload_problem(p)
        out = c.newton(**nr.path_options("through"))
        searched = c.newton(**nr.path_options("inversion72"))
        _, _, flagged = c.internal_force(worst)
        _, _, sound = c.internal_force(out["u"])
    print("through inverted states: newton_iterations", out["newton_iterations"], "the twin's", want["newton_iterations"], "inverted", out["inverted"],
          "smallest det F of the returned state", out["elem"][:, 6].min(), "the twin's worst iterate", det)
    assert out["converged"] == 1 and out["inverted"] == 1 and "message" not in out
    assert np.array_equal(out["newton_iterations"], want["newton_iterations"]) and (out["step_lengths"] == 1.0).all()
    assert out["elem"][:, 6].min() > 0
    assert flagged and not sound
    within_the_bound("through inverted states:", p, out["u"], nr.path_floor("through"))
    assert searched["converged"] == 1 and searched["inverted"] == 0 and searched["halvings"] == 2


# ---- 4. device buffers on an early-ended run
def test_an_early_ended_run_in_device_memory(built):
    """host against device memory, the doubles on an 8-byte boundary that is no 16-byte one: the same bits, every buffer of exactly
    info[3] entries or increments + 1 rows between its guard bands"""
    p, opts = nr.path_problem("early"), nr.path_options("early")
    n2 = 2 * p.mesh.num_nodes
    probes = np.arange(n2 - 1, -1, -3)
    factors = np.array(opts["load_factors"])
    out = {}
    with DeviceArena() as arena, Context(device=0) as host, Context(device=0) as dev:
        for key, leg in (("host", NewtonLeg(host, MAG_MEM_HOST)), ("device", NewtonLeg(dev, MAG_MEM_DEVICE, arena, 8))):
            leg.ctx.upload_problem(p)
            assert leg.run_newton(3, factors.copy(), None, probes.copy(), snapshots=1, max_newton=opts["max_newton"]) == MAG_OK, leg.error()
            assert "increment 3 " in leg.error()
            out[key] = leg.download_newton()
        arena.check()
    got, want = out["device"], out["host"]
    assert list(got) == list(want)
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
        assert np.isfinite(got[k]).all(), k
    assert got["info"][0] == 2 and got["info"][3] == 12 and got["info"][7] == 0
    assert got["newton_iterations"].tolist() == [0, 4, 4, 0] and got["load"].tolist() == [0.0, 0.125, 0.25, 0.0]
    assert got["residuals"].shape == got["step_lengths"].shape == got["cg_iterations"].shape == (12,)
    assert got["probe_u"].shape == (4, len(probes)) and got["snapshots"].shape == (4, n2)
    assert not got["probe_u"][3].any() and not got["snapshots"][3].any() and not got["energies"][3].any()
    assert np.array_equal(got["probe_u"][2], got["u_out"][probes]) and np.array_equal(got["snapshots"][2], got["u_out"])
