"""GPU: the paths of mag_run_transient that tests/test_transient_gpu.py does not reach -- starts that move (u0 and v0 given, NaN on
every prescribed DOF), the stop rule and cg_tol (iteration counts against the stop rule's twin), the iteration cap, the poll
block, the records at their awkward shapes, the refusals of the download, and runs resumed in three segments.

References.  The LU twin of tests/transient_ref.py, and its newmark() with cg_solver(): field_cg_ref.fused_cg, k_cg_field's
recurrence launch by launch under MAG_STOP_REL, which gives the iteration count of every solve and, at a cap, the last iterate.
tests/test_transient.py holds both twins against each other on the CPU: at every (mesh, dt) pair used here the emulation meets
a tenth of the bars below (plate16 at T1 / 200: 1.7e-13 | 5.7e-12; plate16 at T1 / 20: 7.4e-11 | 1.5e-10; holes3k at T1 / 200:
2.8e-13 | 1.5e-11, for u | v, a, f).  No case steps at dt >= T1: there the stop rule's own error reaches 5e-5 in u and neither
twin is a reference.

Bars.  u within TOL_U = 1e-8, v, a and the reactions within TOL_F = 1e-7, relative L2 at every step (check_against_the_twin);
iteration counts within one of the twin's, never equal by assertion (rounding-sized noise moves a count by one at 1 or 2 of 17
steps at T1 / 20); everything that is a copy, a repeat, another poll block or a resumed run: bit for bit.

Meshes: plate16 (289 nodes: 2N = 578, three blocks of 256 threads) and holes3k (shuffled); at most 32 steps; dt = T1 / 200, the
cap's tests T1 / 20 (a step's solve then needs 130 to 160 iterations and the a_0 solve 26 to 37: a cap of 40 stops the one and
not the other).

Measured on an MI355X, at worst over the cases of a group (bar in brackets):
  moving starts (27 cases)    u 2.9e-12 (1e-8), v 1.5e-11, a 1.6e-11, reactions 1.9e-12 (1e-7)
  iteration counts            0 of 408 rows (8 cases x 3 tolerances x 17 solves) one iteration from the twin, none further
  the cap (12 cases)          u 9.2e-13 (1e-8), v 3.9e-13, a 3.4e-13, reactions 3.0e-13 (1e-7) against the capped twin;
                              cg 1 against cg 4: u 1.0e-13, v 3.9e-14, a 1.1e-13, reactions 5.0e-14 -- both phases hand on x_cap
  energies (8 cases)          T 7.4e-14, W 5.1e-14, P 8.1e-13 (1e-7)
A cap off by one would stand at 1e-5 .. 1e-2 (tests/test_transient.py), the start's terms at 1e-1 and more.

That the tests can fail.  One numeric change at a time in a scratch copy of csrc/api.hip / csrc/transient.hip (arithmetic, or a row
that is in bounds; never a bound, a size or a launch shape), built and run against this file and the transient test of
tests/test_device_memory_gpu.py; the tests that then fail (cases failing / cases):
  r.cb = 0 in place of eta at the start      moving_starts 12 / 24 (the damped ones) + 2 / 3, the_iteration_cap 12 / 12, energies 4 / 8
  d_v0 ignored                               moving_starts 24 / 24 + 2 / 3 (all but "u0 only"), the_iteration_cap 12 / 12, energies 8 / 8,
                                             iteration_counts 1 / 8
  u0 read on the prescribed DOFs (NaN)       every test that passes a start: 70 of the 71 cases (the solve breaks down, by name)
  1e-10 whatever cg_tol says                 iteration_counts 8 / 8, the_iteration_cap 4 / 12
  snapshot row (n + 1) / se + 1, the last    snapshot_rows 3 / 4 ((3, 5) keeps row 0 only), three_segments, device memory
    wrapped to row 0 to stay in bounds
  amp_first not restored on resume           three_segments, a_resumed_run_without_an_amplitude, device memory
  probe_v's offset pb replaced by 0          moving_starts 24 / 24 + 2 / 3 (row 0, where v0 is given), the_iteration_cap 12 / 12, probes_repeated_and_unordered
                                             (not the device-memory test: both legs copy the same wrong rows)"""
import ctypes as C
import functools

import numpy as np
import pytest

import modal_ref
import test_transient_gpu as tg
import transient_ref as ref
from magnetite_amd import Context, _lib
from magnetite_amd._lib import MAG_OK
from test_load_cases_gpu import TOL_F, assert_case_equals, rel
from test_transient_gpu import CG_TOL, RHO, amplitude_of, assert_same_bits, check_against_the_twin, every_step, parameters

pytestmark = pytest.mark.gpu

MAG_ERR_STATE = 7
KIND = {0: 3, 1: 1, 2: 2, 3: 3, 4: 1}  # the twin's kind of the device's cg (4, the CSR phase, is plain CG)
STATE = ("u", "v", "a", "f")


# ---- what the tests share: computed once, left unchanged
@functools.lru_cache(maxsize=None)
def start(name, config, lumped=False):
    """(u0, v0) of transient_ref.moving_start: modes 2 and 3, NaN on every prescribed DOF"""
    prob, K, M, free, w1, T1 = tg.setup(name, config, lumped)
    lam, Phi = modal_ref.eigenpairs(K, M, free, 4)
    return ref.moving_start(K, M, free, prob.u_in, prob.f_in, Phi, 0.05 * w1, 0.02 / w1)


def case(name, config, which, steps, per_period=200, lumped=False, given="both", load="sine"):
    """everything a run and its twin need: (prob, dict(dt, amplitude, u0, v0), dict(beta, gamma, rayleigh))"""
    prob, K, M, free, w1, T1 = tg.setup(name, config, lumped)
    beta, gamma, alpha, eta = parameters(which, w1)
    dt = T1 / per_period
    u0, v0 = start(name, config, lumped)
    run = dict(dt=dt, amplitude=amplitude_of(config, dt, T1, steps) if load == "sine" else None,
               u0=u0 if given in ("both", "u0") else None, v0=v0 if given in ("both", "v0") else None)
    return prob, run, dict(beta=beta, gamma=gamma, rayleigh=(alpha, eta))


@functools.lru_cache(maxsize=None)
def twin(name, config, which, steps, per_period=200, lumped=False, given="both", load="sine", solver=None):
    """(newmark()'s dict, [(iterations, converged)] of every solve); solver: None for the LU twin, or (kind, tol, max_iter)"""
    prob, K, M, free, w1, T1 = tg.setup(name, config, lumped)
    _, run, par = case(name, config, which, steps, per_period, lumped, given, load)
    log = []
    kw = {} if solver is None else dict(solver=ref.cg_solver(prob.u_known, solver[0], solver[1], solver[2], log))
    out = ref.newmark(K, M, free, prob.u_in, prob.f_in, steps, run["dt"], par["beta"], par["gamma"], *par["rayleigh"], run["amplitude"],
                      run["u0"], run["v0"], **kw)
    return out, log


def rows_of(out):
    """a run with probes at every DOF as check_against_the_twin reads one: the state at every row, the reactions at the last"""
    f = np.full(out["probe_u"].shape, np.nan)
    f[-1] = out["f"]
    return dict(u=out["probe_u"], v=out["probe_v"], a=out["probe_a"], f=f, iterations=out["iterations"])


# ---- 1. moving starts
def moving_start_case(name, config, which, cg, lumped=False, given="both"):
    steps = 16
    prob, run, par = case(name, config, which, steps, lumped=lumped, given=given)
    assert all(x is None or np.isnan(x[np.asarray(prob.u_known) != 0]).all() for x in (run["u0"], run["v0"]))
    want = twin(name, config, which, steps, lumped=lumped, given=given)[0]
    # the twin alone: the start's terms stand above the bars, or the bars would not see them
    if given in ("both", "v0"):
        other = twin(name, config, which, steps, lumped=lumped, given={"both": "u0", "v0": "none"}[given])[0]
        assert which == "undamped" or rel(other["a"][0], want["a"][0]) >= 1e-2
        assert rel(other["f"][1], want["f"][1]) >= 1e-2
    if given in ("both", "u0"):
        other = twin(name, config, which, steps, lumped=lumped, given={"both": "v0", "u0": "none"}[given])[0]
        assert rel(other["a"][0], want["a"][0]) >= 1e-2
    with Context(device=0) as c:
        out = every_step(c, prob, steps, cg=cg, lumped=lumped, **run, **par)
    assert not np.isnan(out["u"]).any() and not np.isnan(out["v"]).any() and not np.isnan(out["a"]).any()
    return check_against_the_twin(out, want, (name, config, which, cg, lumped, given))


@pytest.mark.parametrize("name", ["plate16", "holes3k"])
@pytest.mark.parametrize("config", ["load", "pull"])
@pytest.mark.parametrize("which", ["undamped", "damped"])
@pytest.mark.parametrize("cg", [1, 3, 4])
def test_moving_starts_against_the_twin(built, name, config, which, cg):
    moving_start_case(name, config, which, cg)


@pytest.mark.parametrize("lumped, given, cg", [(True, "both", 3), (False, "v0", 2), (False, "u0", 4)])
def test_moving_starts_lumped_and_with_one_vector_only(built, lumped, given, cg):
    moving_start_case("holes3k", "load", "damped", cg, lumped, given)


# ---- 2. the stop rule and cg_tol
@pytest.mark.parametrize("config", ["load", "pull"])
@pytest.mark.parametrize("cg", [1, 2, 3, 4])
def test_iteration_counts_against_the_stop_rules_twin(built, config, cg):
    steps = 16
    prob, run, par = case("plate16", config, "damped", steps)
    want = {tol: np.array([n for n, _ in twin("plate16", config, "damped", steps, solver=(KIND[cg], tol, 10 ** 7))[1]])
            for tol in (1e-6, 1e-10, 1e-12)}
    assert np.all(want[1e-6] < want[1e-12])
    assert np.all(want[1e-10] <= want[1e-12] - 3) and np.all(want[1e-6] <= want[1e-10] - 3)  # (the default is told from both)
    got = {}
    with Context(device=0) as c:
        c.upload_problem(prob)
        for cg_tol in (1e-6, 1e-12, 0.0):
            out = c.transient(steps=steps, density=RHO, cg=cg, cg_tol=cg_tol, **run, **par)
            got[cg_tol] = out["iterations"]
            off = np.abs(out["iterations"] - want[cg_tol or 1e-10])
            print("plate16", config, "cg", cg, "cg_tol", cg_tol, "rows one iteration from the twin:", int(np.count_nonzero(off == 1)), "of", steps + 1,
                  "further:", int(np.count_nonzero(off > 1)))
            assert out["converged"] == 1 and out["iterations"].shape == (steps + 1,)
            assert off.max() <= 1, (cg_tol, out["iterations"], want[cg_tol or 1e-10])
            assert out["cg_iterations"] == int(out["iterations"].sum()) and out["max_step_iterations"] == int(out["iterations"].max())
    assert np.all(got[1e-6] < got[1e-12])


# ---- 3. the cap
CAPS = {5: {}, 9: dict(check_every=2), 40: dict(check_every=2)}  # 5: inside the first poll block; 9: odd, behind it; 40: several


@functools.lru_cache(maxsize=None)
def capped(cap, cg):
    """8 steps under max_iter = cap: the run as one, as 4 + 4 resumed, the message, and a static run on the context afterwards"""
    steps = 8
    prob, run, par = case("plate16", "load", "damped", steps, per_period=20)
    n2 = 2 * prob.mesh.num_nodes
    kw = dict(density=RHO, probes=np.arange(n2), cg=cg, cg_tol=CG_TOL, dt=run["dt"], **par)
    with Context(device=0, max_iter=cap, **CAPS[cap]) as c:
        c.upload_problem(prob)
        status = c.run_transient(steps, amplitude=run["amplitude"], u0=run["u0"], v0=run["v0"], **kw)
        message = c._L.mag_last_error(c._h).decode()
        whole = dict(c.download_transient(), **c.transient_info())
        max_iter = c.options.max_iter
        c.run()
        static = dict(zip(("u", "f", "stress"), c.download()), **c.stats())
        head = c.transient(steps=4, amplitude=run["amplitude"][:5], u0=run["u0"], v0=run["v0"], **kw)
        tail = c.transient(steps=4, amplitude=run["amplitude"][4:], resume=True, **kw)
    return dict(status=status, message=message, whole=whole, max_iter=max_iter, static=static, head=head, tail=tail)


@pytest.mark.parametrize("cap", list(CAPS))
@pytest.mark.parametrize("cg", [1, 2, 3, 4])
def test_the_iteration_cap_hands_on_the_last_iterate(built, cap, cg):
    steps = 8
    prob = case("plate16", "load", "damped", steps, per_period=20)[0]
    want, log = twin("plate16", "load", "damped", steps, per_period=20, solver=(KIND[cg], CG_TOL, cap))
    # the twin alone: a solve either stops two iterations short of the cap or would run two beyond it -- no row is in doubt
    stopped = np.array([done == 0 for _, done in log])
    assert stopped.any() and all(n == cap for n, done in log if not done) and all(n <= cap - 2 for n, done in log if done)
    beyond = twin("plate16", "load", "damped", steps, per_period=20, solver=(KIND[cg], CG_TOL, cap + 2))[1]
    assert [done == 0 for _, done in beyond] == stopped.tolist()
    got = capped(cap, cg)
    out = got["whole"]
    assert got["status"] == MAG_OK and out["converged"] == 0
    assert "mag_run_transient" in got["message"] and "iteration cap" in got["message"] and "last iterate" in got["message"]
    counts = np.array([n for n, _ in log])
    assert np.array_equal(out["iterations"][stopped], counts[stopped]), (out["iterations"], counts)
    assert np.abs(out["iterations"] - counts).max() <= 1 and out["max_step_iterations"] == cap
    assert out["cg_iterations"] == int(out["iterations"].sum())
    check_against_the_twin(rows_of(out), want, ("cap", cap, "cg", cg))
    # the context is as it was: its own run stops at its own cap, as on a context that never saw the pass
    assert got["max_iter"] == cap
    with Context(device=0, max_iter=cap, **CAPS[cap]) as fresh:
        assert_case_equals(fresh.solve(prob), got["static"], "a run after the capped pass")
    assert got["static"]["iterations"] == cap and got["static"]["converged"] == 0
    # 4 + 4 steps resumed: the bits of the 8
    head, tail = got["head"], got["tail"]
    for k in ("probe_u", "probe_v", "probe_a"):
        assert np.array_equal(head[k], out[k][:5]) and np.array_equal(tail[k], out[k][4:]), k
    for k in STATE:
        assert np.array_equal(tail[k], out[k]), k
    assert np.array_equal(head["iterations"], out["iterations"][:5]) and np.array_equal(tail["iterations"][1:], out["iterations"][5:])
    assert head["converged"] == 0 and tail["converged"] == 0 and tail["iterations"][0] == 0


@pytest.mark.parametrize("cap", list(CAPS))
def test_both_phases_hand_on_the_same_iterate_at_the_cap(built, cap):
    fused, csr = rows_of(capped(cap, 1)["whole"]), rows_of(capped(cap, 4)["whole"])
    check_against_the_twin(fused, csr, ("cap", cap, "cg 1 against cg 4"))


# ---- 4. the poll does not matter
@pytest.mark.parametrize("name", ["plate16", "holes3k"])
@pytest.mark.parametrize("cg", [0, 4])
def test_no_result_depends_on_the_poll_block(built, name, cg):
    steps = 16
    prob, run, par = case(name, "load", "damped", steps)
    outs = []
    for check_every in (2, 64, 4096):
        with Context(device=0, check_every=check_every) as c:
            outs.append(c.transient(prob, steps=steps, density=RHO, probes=np.arange(2 * prob.mesh.num_nodes), energies=True, snapshot_every=4,
                                    cg=cg, cg_tol=CG_TOL, **run, **par))
    assert outs[0]["converged"] == 1 and outs[0]["iterations"].min() > 2
    assert_same_bits(outs[0], outs[1], "check_every 2 and 64")
    assert_same_bits(outs[0], outs[2], "check_every 2 and 4096")


# ---- 5. records
@pytest.mark.parametrize("steps, every", [(10, 4), (3, 5), (1, 1), (7, 7)])
def test_snapshot_rows(built, steps, every):
    prob, run, par = case("plate16", "load", "damped", steps)
    n2 = 2 * prob.mesh.num_nodes
    with Context(device=0) as c:
        out = c.transient(prob, steps=steps, density=RHO, probes=np.arange(n2), snapshot_every=every, cg_tol=CG_TOL, **run, **par)
    kept = steps // every + 1
    assert out["snapshots_kept"] == kept and out["snapshots"].shape == (kept, n2) and out["probe_u"].shape == (steps + 1, n2)
    for j in range(kept):
        assert np.array_equal(out["snapshots"][j], out["probe_u"][j * every]), j
    assert len({out["probe_u"][n].tobytes() for n in range(steps + 1)}) == steps + 1  # (every step another state)


def some_probes(prob, count=300, seed=300):
    """`count` DOFs with repeats, in no order, among them 0, 2N - 1, a support and the loaded DOF"""
    n2 = 2 * prob.mesh.num_nodes
    probes = np.random.default_rng(seed).integers(0, n2, count)
    probes[[0, 1, 2, 3, 4]] = n2 - 1, 0, np.flatnonzero(np.asarray(prob.u_known) != 0)[3], np.flatnonzero(np.asarray(prob.f_in) != 0)[0], n2 - 1
    assert len(set(probes.tolist())) < count and np.any(np.diff(probes) < 0)
    return probes.astype(np.int32)


def test_probes_repeated_and_unordered_across_a_block(built):
    steps = 10
    prob, run, par = case("plate16", "load", "damped", steps)
    n2 = 2 * prob.mesh.num_nodes
    probes = some_probes(prob)
    assert n2 // 256 < (n2 + len(probes)) // 256  # (the probes' threads reach into another block of 256)
    with Context(device=0) as c:
        every = c.transient(prob, steps=steps, density=RHO, probes=np.arange(n2), cg_tol=CG_TOL, **run, **par)
        out = c.transient(steps=steps, density=RHO, probes=probes, cg_tol=CG_TOL, **run, **par)
    for k in ("u", "v", "a"):
        assert out["probe_" + k].shape == (steps + 1, len(probes))
        assert np.array_equal(out["probe_" + k], every["probe_" + k][:, probes]), k
        assert np.array_equal(out["probe_" + k][-1], out[k][probes]), k
    assert not np.array_equal(every["probe_u"], every["probe_v"]) and not np.array_equal(every["probe_v"], every["probe_a"])
    for k in STATE + ("iterations",):
        assert np.array_equal(out[k], every[k]), k


@pytest.mark.parametrize("name", ["plate16", "holes3k"])
@pytest.mark.parametrize("config, which", [("load", "damped"), ("pull", "undamped")])
@pytest.mark.parametrize("lumped", [False, True], ids=["consistent", "lumped"])
def test_energies_against_the_twin(built, name, config, which, lumped):
    steps = 16
    loads = ("sine", "constant") if config == "load" else ("sine",)
    for load in loads:
        prob, run, par = case(name, config, which, steps, lumped=lumped, load=load)
        want = twin(name, config, which, steps, lumped=lumped, load=load)[0]["energies"]
        with Context(device=0) as c:
            out = c.transient(prob, steps=steps, density=RHO, energies=True, lumped=lumped, cg_tol=CG_TOL, **run, **par)
        got = out["energies"]
        assert got.shape == (steps + 1, 3) and out["converged"] == 1
        worst = {}
        for col, k in enumerate("TWP"):
            rows = want[:, col] != 0.0
            if config == "pull" and k == "P":  # no load: identically zero, and no -0
                assert not rows.any() and not got[:, col].any() and not np.signbit(got[:, col]).any()
                continue
            assert rows.sum() >= steps
            worst[k] = rel(got[rows, col], want[rows, col])
        print(name, config, which, "lumped" if lumped else "consistent", load, "energies against the twin", worst)
        assert max(worst.values()) <= TOL_F, worst
        if load == "constant":  # under a constant load damping only takes: T + W - P never rises (of the twin first)
            for e in (want, got):
                balance = e[:, 0] + e[:, 1] - e[:, 2]
                assert np.diff(balance).max() <= 1e-8 * e[:, 1].max()
            assert balance[-1] < balance[0] - 1e-3 * got[:, 1].max()


def test_the_download_refuses_what_the_run_did_not_record_and_skips_null_members(built):
    steps = 6
    prob, run, par = case("plate16", "load", "damped", steps)
    n2 = 2 * prob.mesh.num_nodes
    x = np.full(3 * (steps + 1) * n2, 7.0)
    with Context(device=0) as c:
        bare = c.transient(prob, steps=steps, density=RHO, cg_tol=CG_TOL, **run, **par)
        assert not {"probe_u", "probe_v", "probe_a", "energies", "snapshots"} & set(bare) and bare["snapshots_kept"] == 0
        for member, words in (("probe_u", b"recorded no probes"), ("probe_v", b"recorded no probes"), ("probe_a", b"recorded no probes"),
                              ("energies", b"recorded no energies"), ("snapshots", b"kept no snapshots")):
            o = _lib.TransientResult(**{member: x.ctypes.data})
            assert c._L.mag_download_transient(c._h, C.byref(o)) == MAG_ERR_STATE, member
            assert b"mag_download_transient" in c._L.mag_last_error(c._h) and words in c._L.mag_last_error(c._h), member
            assert (x == 7.0).all()
            again = c.download_transient()  # the run's other results stay
            assert list(again) == [k for k in bare if k in again]
            for k in again:
                assert np.array_equal(again[k], bare[k]), (member, k)
        full = c.transient(steps=steps, density=RHO, probes=np.arange(n2), energies=True, snapshot_every=2, cg_tol=CG_TOL, **run, **par)
        part = c.download_transient(num_probes=0, energies=False)
    assert set(full) - set(part) == {"probe_u", "probe_v", "probe_a", "energies"} | set(Context.TRANSIENT_INFO)
    for k in part:
        assert np.array_equal(part[k], full[k]), k
    for k in STATE + ("iterations",):
        assert np.array_equal(full[k], bare[k]), k  # (the records change nothing)


# ---- 6. resume
def test_three_segments_with_other_records_in_the_middle(built):
    steps, cuts = 32, (1, 23)
    prob, run, par = case("plate16", "load", "damped", steps)
    n2 = 2 * prob.mesh.num_nodes
    dt, amp = run["dt"], run["amplitude"]
    other = some_probes(prob, 11, seed=5)
    every = dict(probes=np.arange(n2), energies=True, snapshot_every=4)
    kw = dict(dt=dt, density=RHO, cg_tol=CG_TOL, **par)

    def ignored_first(a):
        a = a.copy()
        a[0] = np.nan  # (a resumed run's amplitude[0] is ignored)
        return a

    with Context(device=0) as c:
        whole = c.transient(prob, steps=steps, amplitude=amp, u0=run["u0"], v0=run["v0"], **every, **kw)
        one = c.transient(steps=1, amplitude=amp[:2], u0=run["u0"], v0=run["v0"], **every, **kw)
        two = c.transient(steps=22, amplitude=ignored_first(amp[1:24]), resume=True, probes=other, snapshot_every=3, **kw)
        three = c.transient(steps=9, amplitude=ignored_first(amp[23:]), resume=True, **every, **kw)
    assert whole["converged"] == 1 and (one["resumed"], two["resumed"], three["resumed"]) == (0, 1, 1)
    for k in STATE:
        assert np.array_equal(three[k], whole[k]), k
    for seg, first, last, dofs in ((one, 0, 1, np.arange(n2)), (two, 1, 23, other), (three, 23, 32, np.arange(n2))):
        for k in ("probe_u", "probe_v", "probe_a"):
            assert np.array_equal(seg[k], whole[k][first:last + 1][:, dofs]), (first, k)
        assert seg["iterations"].shape == (last - first + 1,) and np.array_equal(seg["iterations"][1:], whole["iterations"][first + 1:last + 1])
        assert seg["iterations"][0] == (whole["iterations"][0] if first == 0 else 0) and whole["iterations"][0] > 0
    assert "energies" not in two
    assert np.array_equal(one["energies"], whole["energies"][:2]) and np.array_equal(three["energies"], whole["energies"][23:])
    assert not np.isnan(whole["energies"]).any()
    # a segment's snapshots are its own steps 0, k, 2k, ...: whole's state at the same global step (through its probes)
    for seg, first, k, kept in ((one, 0, 4, 1), (two, 1, 3, 8), (three, 23, 4, 3)):
        assert seg["snapshots_kept"] == kept and seg["snapshots"].shape == (kept, n2)
        for j in range(kept):
            assert np.array_equal(seg["snapshots"][j], whole["probe_u"][first + j * k]), (first, j)
    assert (one["t_start"], one["t_end"]) == (0.0, dt) and (two["t_start"], two["t_end"]) == (one["t_end"], one["t_end"] + 22 * dt)
    assert (three["t_start"], three["t_end"]) == (two["t_end"], two["t_end"] + 9 * dt)


def test_a_resumed_run_without_an_amplitude_records_the_load_it_resumes(built):
    prob, run, par = case("plate16", "load", "damped", 2)
    n2 = 2 * prob.mesh.num_nodes
    loaded = int(np.flatnonzero(np.asarray(prob.f_in) != 0)[0])
    assert np.count_nonzero(prob.f_in) == 1 and not prob.u_known[loaded]
    kw = dict(dt=run["dt"], density=RHO, probes=np.arange(n2), energies=True, cg_tol=CG_TOL, **par)
    with Context(device=0) as c:
        first = c.transient(prob, steps=2, amplitude=np.array([1.0, 1.3, 1.7]), u0=run["u0"], v0=run["v0"], **kw)
        second = c.transient(steps=2, resume=True, **kw)
    work = prob.f_in[loaded] * second["probe_u"][:, loaded]  # f . u_F has this one term
    assert np.array_equal(second["energies"][0], first["energies"][2])
    assert np.allclose(second["energies"][:, 2], np.array([1.7, 1.0, 1.0]) * work, rtol=1e-14, atol=0.0) and np.all(work != 0.0)
