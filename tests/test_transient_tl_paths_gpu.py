"""GPU: the paths of mag_run_transient_tl that tests/test_transient_tl_gpu.py only brushes, on the cases of transient_tl_cases'
EARLY / LONG / INVERTED / NEWMARK (admitted on the CPU in tests/test_transient_tl.py: every integer asked of the device here is
off its threshold on the twin) -- a run that ends early after converged steps (the probe blocks' compaction, the shortened
records, the amplitude of the last converged step, the time, the snapshots kept), its resumed continuation under an amplitude, an
inverted trial state, Newmark parameters other than (1/4, 1/2) with damping and both masses, device buffers on an early-ended run.

The case: plate16 / load300 at its own dt, 8 steps, amplitude 1, 1.01, 1.02, 1.03, then 18 at row 4 and 24 behind it
(transient_tl_cases.jump).  With max_newton = 5 steps 1..3 converge (5, 4, 4 iterations) and step 4 stands at 2e-6 at the cap;
with max_newton = 6 all 8 steps converge.  A jump to 100 inverts a trial state of step 4.

Bars (the project's own, tests/test_transient_tl_gpu.py): integers and shapes equal the twin's; "the same bits" is tobytes()
equality of two device runs; u within 1e-8, v, a, reactions, probes and energies within 1e-7 of the twin run on to its floor
(extra = 3); the element rows 1e-12; residual ratios above 1e-8 within rel 1e-4.  Every test prints its figures before it asserts.

Measured on an MI355X (TT-paths): the early end -- 3 steps, newton_iterations [0, 5, 4, 4], 18 residuals, step 4 at
2.105e-06 at the cap, rows 0..3 and both snapshots the bits of the 8-step run ([0, 5, 4, 4, 6, 5, 4, 4, 4]), the state the bits of a
3-step run, u 5.4e-13, v 6.8e-13, a 4.4e-13 from the twin's floor run; both resumes the 8-step run's rows 3..8 bit for bit; the
jump to 100: 3 steps, inverted = 1, 2.043e-01 at the cap; the four Newmark cases with and without the tables: the twin's counts
(3 a step; 4 in step 1 of load300), u at most 8.9e-14, every other figure at most 6.6e-12 (bars 1e-8 / 1e-7), the element rows
2.1e-16, and 6.4e-3 to 0.18 from the (1/4, 1/2) runs."""
import numpy as np
import pytest

import transient_tl_cases as cases
from device_buffers import DeviceArena
from magnetite_amd import Context
from magnetite_amd._lib import MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK
from test_transient_tl_gpu import CONTEXTS, RHO, SET, TransientTlLeg, check_against_the_twin, device_run, rel

pytestmark = pytest.mark.gpu

NAME, KIND = "plate16", "load300"
STATE = ("u", "v", "a", "f", "elements")
ROWS = ("probe_u", "probe_v", "probe_a", "energies")


def amplitude(which):
    return cases.jump(which["jump_to"], which.get("jump_then"))


def the_case():
    s = cases.setup(NAME, KIND)
    p = s["prob"]
    n2 = 2 * p.mesh.num_nodes
    probes = np.arange(0, n2, 5)
    kw = dict(dt=s["dt"], density=RHO, probes=probes, energies=True, snapshot_every=2, kinematics="tl", **SET)
    return s, p, n2, probes, kw


# ---- 1. an early end after converged steps
@CONTEXTS
def test_an_early_end_keeps_the_converged_steps(built, context):
    s, p, n2, probes, kw = the_case()
    dt, amp, cap = s["dt"], amplitude(cases.EARLY), cases.EARLY["max_newton"]
    known = np.asarray(p.u_known).reshape(-1) != 0
    with Context(device=0, **context) as c:
        c.upload_problem(p)
        long = c.transient(steps=8, amplitude=amp, max_newton=cases.LONG["max_newton"], **kw)
        three = c.transient(steps=3, amplitude=amp[:4], max_newton=cap, **kw)
        out = c.transient(steps=8, amplitude=amp, max_newton=cap, **kw)
    print(context, "early end:", out["message"], "newton_iterations", out["newton_iterations"], "cg", out["iterations"], "the long run's newton_iterations",
          long["newton_iterations"], "residuals of the step at the cap", out["newton_residuals"][13:])
    assert out["steps"] == 3 and out["converged"] == 0 and out["resumed"] == 0 and not out["inverted"]
    assert out["t_start"] == 0.0 and out["t_end"] == 3 * dt
    assert out["newton_iterations"].tolist() == [0, 5, 4, 4] and len(out["iterations"]) == 4 and out["max_step_newton"] == 5
    assert out["newton_iterations_total"] == len(out["newton_residuals"]) == len(out["newton_cg"]) == 18
    assert out["cg_iterations"] == out["iterations"].sum() and out["max_step_iterations"] == out["iterations"].max()
    assert out["newton_cg"][:13].sum() + out["iterations"][0] == out["iterations"].sum()  # (the step at the cap is in no row)
    for k in ("probe_u", "probe_v", "probe_a"):
        assert out[k].shape == (4, len(probes)), k
    assert out["energies"].shape == (4, 3) and out["snapshots"].shape == (2, n2) and out["snapshots_kept"] == 2
    assert "step 4 " in out["message"] and "5 iterations" in out["message"] and "mag_run_transient_tl" in out["message"]
    assert out["newton_residuals"][-1] > 100 * cases.NEWTON_TOL
    # the rows of the converged steps are the long run's: the check of the block move
    assert long["converged"] == 1 and long["steps"] == 8 and long["newton_iterations"].tolist() == [0, 5, 4, 4, 6, 5, 4, 4, 4]
    for k in ROWS + ("iterations", "newton_iterations"):
        assert out[k].tobytes() == long[k][:4].tobytes(), k
    assert out["snapshots"].tobytes() == long["snapshots"][:2].tobytes()
    for k in ("newton_residuals", "newton_cg"):
        assert out[k][:13].tobytes() == long[k][:13].tobytes(), k
    for k in ("u", "v", "a"):
        assert out[k][probes].tobytes() == long["probe_" + k][3].tobytes(), k
        assert out["probe_" + k][3].tobytes() == out[k][probes].tobytes(), k
    assert out["snapshots"][1].tobytes() != out["u"].tobytes() and np.array_equal(out["snapshots"][1][probes], out["probe_u"][2])
    # the state, the reactions and the element rows are a three-step run's
    assert three["converged"] == 1 and three["steps"] == 3
    for k in STATE:
        assert out[k].tobytes() == three[k].tobytes(), k
    for k in ROWS:
        assert out[k].tobytes() == three[k].tobytes(), k
    assert np.array_equal(out["f"][~known], (amp[3] * np.asarray(p.f_in))[~known])  # (amplitude[steps done], not amplitude[steps])
    # against the twin
    want = cases.twin_with(NAME, KIND, **cases.EARLY)
    floor = cases.twin_with(NAME, KIND, extra=3, steps=3, jump_to=cases.EARLY["jump_to"], jump_then=cases.EARLY["jump_then"])
    assert want["steps_done"] == out["steps"] and not want["converged"] and not want["inverted"]
    assert np.array_equal(out["newton_iterations"], want["newton_iterations"])
    early = want["residuals"] > 1e-8
    err = {k: rel(out[k], floor[k][-1]) for k in ("u", "v", "a")}
    err["residuals"] = rel(out["newton_residuals"][early], want["residuals"][early])
    print(context, "early end against the twin's floor run of three steps:", " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert err["u"] <= 1e-8 and max(err["v"], err["a"]) <= 1e-7 and err["residuals"] <= 1e-4
    check_against_the_twin(p, three, cases.twin_with(NAME, KIND, steps=3, jump_to=cases.EARLY["jump_to"], jump_then=cases.EARLY["jump_then"]), floor,
                           probes, (NAME, "the three-step run", context), amp_last=amp[3])


# ---- 2. resume after an early end, under an amplitude
def continues(what, long, first, rest, probes, dt):
    """`rest` (5 steps, resumed behind the 3 of `first`) against the 8 steps of `long`: bit for bit"""
    assert rest["resumed"] == 1 and rest["converged"] == 1 and rest["steps"] == 5 and rest["iterations"][0] == 0, what
    assert rest["t_start"] == first["t_end"] == 3 * dt and rest["t_end"] == long["t_end"], what
    for k in ("u", "v", "a"):
        assert rest["probe_" + k][0].tobytes() == first[k][probes].tobytes(), (what, k)
    assert rest["energies"][0].tobytes() == first["energies"][3].tobytes(), what  # (P of row 0: the amplitude of the resumed state)
    for k in STATE:
        assert rest[k].tobytes() == long[k].tobytes(), (what, k)
    for k in ROWS:
        assert rest[k].tobytes() == long[k][3:].tobytes(), (what, k)
    assert np.array_equal(rest["newton_iterations"][1:], long["newton_iterations"][4:]), what
    assert np.array_equal(rest["iterations"][1:], long["iterations"][4:]), what
    assert rest["snapshots"].shape == (3, len(rest["u"])), what
    for k in range(3):  # (its snapshots are of its own steps 0, 2, 4: the long run's 3, 5, 7)
        assert rest["snapshots"][k][probes].tobytes() == long["probe_u"][3 + 2 * k].tobytes(), (what, k)


def test_a_resume_after_an_early_end_under_an_amplitude(built):
    """amplitude[0] of a resumed run is ignored (the header): row 0 carries the amplitude of the state resumed, here 1.03, whatever
    is passed -- after an early end (read back from amplitude[steps done]) and after a completed run (amplitude[steps])"""
    s, p, n2, probes, kw = the_case()
    dt, amp = s["dt"], amplitude(cases.EARLY)
    stale = amp[3:].copy()
    stale[0] = -7.0
    with Context(device=0) as c:
        c.upload_problem(p)
        long = c.transient(steps=8, amplitude=amp, max_newton=6, **kw)
        early = c.transient(steps=8, amplitude=amp, max_newton=5, **kw)
        after_early = c.transient(steps=5, resume=True, amplitude=stale, max_newton=6, **kw)
        first = c.transient(steps=3, amplitude=amp[:4], max_newton=6, **kw)
        after_first = c.transient(steps=5, resume=True, amplitude=amp[3:], max_newton=6, **kw)
    print("resumed behind the early end: newton", after_early["newton_iterations"], "behind three steps:", after_first["newton_iterations"], "the long run's",
          long["newton_iterations"])
    assert early["converged"] == 0 and early["steps"] == 3 and first["converged"] == 1 and long["converged"] == 1
    continues("behind the early end", long, early, after_early, probes, dt)
    continues("behind three steps", long, first, after_first, probes, dt)


# ---- 3. an inverted trial state
def test_an_inverted_trial_state_raises_the_flag_and_is_no_error(built):
    s, p, n2, probes, kw = the_case()
    want = cases.twin_with(NAME, KIND, **cases.INVERTED)
    with Context(device=0) as c:
        c.upload_problem(p)
        rc = c.run_transient_tl(8, s["dt"], RHO, amplitude=amplitude(cases.INVERTED), probes=probes, energies=True, max_newton=5, **SET)
        info, out, own = c.transient_tl_info(), c.download_transient(), c.download_transient_tl()
        message = c._L.mag_last_error(c._h).decode()
    print("inverted trial:", message, "info", info, "the twin's smallest det F", want["min_det"], "its steps", want["steps_done"])
    assert rc == MAG_OK and want["inverted"] and want["min_det"] < -1.0 and not want["converged"]
    assert info["inverted"] == 1 and info["converged"] == 0 and info["steps"] == want["steps_done"] == 3
    assert np.array_equal(own["newton_iterations"], want["newton_iterations"]) and "step 4 " in message
    assert own["elements"][:, 6].min() > 0 and all(np.isfinite(out[k]).all() for k in out if k not in ("t_start", "t_end"))
    floor = cases.twin_with(NAME, KIND, extra=3, steps=3, jump_to=cases.INVERTED["jump_to"])
    err = {k: rel(out[k], floor[k][-1]) for k in ("u", "v", "a")}
    print("the state kept against the twin's floor run of three steps:", " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert err["u"] <= 1e-8 and max(err["v"], err["a"]) <= 1e-7


# ---- 4. Newmark parameters other than (1/4, 1/2)
@pytest.mark.parametrize("name, kind, beta, gamma, lumped", cases.NEWMARK)
@CONTEXTS
def test_other_newmark_parameters_against_the_twin(built, name, kind, beta, gamma, lumped, context):
    with Context(device=0, **context) as c:
        s, probes, out = device_run(c, name, kind, lumped=lumped, beta=beta, gamma=gamma)
        _, _, plain = device_run(c, name, kind, lumped=lumped)
    kw = dict(lumped=lumped, beta=beta, gamma=gamma)
    check_against_the_twin(s["prob"], out, cases.twin_with(name, kind, **kw), cases.twin_with(name, kind, extra=3, **kw), probes,
                           (name, kind, beta, gamma, "lumped" if lumped else "consistent", context))
    apart = rel(out["u"], plain["u"])
    print(name, kind, beta, gamma, "rel(u, the (1/4, 1/2) run)", apart)
    assert apart > 1e-4  # (the parameters matter)


# ---- 5. device buffers on an early-ended run
def test_an_early_ended_run_in_device_memory(built):
    """host against device memory, the doubles on an 8-byte boundary that is no 16-byte one: the same bits; mag_download_transient
    and mag_download_transient_tl write steps done + 1 rows and info[3] entries, the slack behind them untouched"""
    s, p, n2, probes, _ = the_case()
    amp = amplitude(cases.EARLY)
    out = {}
    with DeviceArena() as arena, Context(device=0) as host, Context(device=0) as dev:
        for key, leg in (("host", TransientTlLeg(host, MAG_MEM_HOST)), ("device", TransientTlLeg(dev, MAG_MEM_DEVICE, arena, 8))):
            leg.ctx.upload_problem(p)
            rc = leg.run_transient_tl(8, s["dt"], RHO, amp.copy(), None, None, probes.copy(), energies=1, snapshot_every=2, max_newton=5, **SET)
            assert rc == MAG_OK, leg.error()
            assert "step 4 " in leg.error()
            out[key, "run"] = leg.download_transient()
            out[key, "own"] = leg.download_transient_tl()
        arena.check()
    for part in ("run", "own"):
        got, want = out["device", part], out["host", part]
        assert list(got) == list(want)
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (part, k)
            assert np.isfinite(got[k]).all(), (part, k)
    run, own = out["device", "run"], out["device", "own"]
    assert own["info"][0] == 3 and own["info"][3] == 18 and own["info"][7] == 0
    assert own["newton_iterations"].tolist() == [0, 5, 4, 4] and own["residuals"].shape == own["cg_iterations"].shape == (18,)
    assert run["probe_u"].shape == run["probe_v"].shape == run["probe_a"].shape == (4, len(probes)) and run["iterations"].shape == (4,)
    assert run["energies"].shape == (4, 3) and run["snapshots"].shape == (2, n2) and run["t_end"] == 3 * s["dt"]
    for k in ("u", "v", "a"):
        assert np.array_equal(run["probe_" + k][3], run[k][probes]), k
    assert np.array_equal(run["snapshots"][1][probes], run["probe_u"][2])
