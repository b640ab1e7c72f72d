"""GPU: mag_run_transient -- Newmark time stepping of the uploaded part on the device -- against the scipy twin of
tests/transient_ref.py (one sparse LU per system) and the closed form of the average-acceleration scheme; the effective matrix
entry by entry; energies, records, the zero state, repeats and resumed runs bit for bit; the fall-back without tile-local tables;
nothing else of the context changes; the refusals that need the device.

Meshes: plate16, holes3k, frontal3k, two_fans of tests/test_load_cases_gpu.py, each as uploaded ("pull": prescribed displacements
on the right edge) and as config_fixed_left_point_load ("load": a force).  Unless said otherwise 64 steps, dt = T1 / 200 with T1
from modal_ref.eigenpairs, cg_tol = 1e-12.

Bars (from the issue): u within TOL_U = 1e-8, v, a and the reactions within TOL_F = 1e-7, relative L2, at every step -- the
project's two parity bars (a CPU emulation of the stop rule stays at or below 6e-10 at this dt); the effective matrix 1e-14 of its
largest entry, (c_K, c_M) = (1, 0) bit for bit; T + W - P constant to 1e-8 of the peak strain energy.  Measured on an MI355X, at
worst over the 64 forced cases: u 4.5e-10, v 5.5e-10, a 2.8e-10, reactions 2.3e-9; the closed form 2.5e-12; the energy drift
1.4e-11; the effective matrix 3.9e-16.

The state at every step is read through probes at every DOF; the reactions of every step by running the steps one at a time,
each a resumed run (which test_repeat_and_resume shows to give the bits of one run)."""
import functools

import numpy as np
import pytest

import modal_ref
import transient_ref as ref
from magnetite_amd import Context, meshgen
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import MESHES, TOL_F, TOL_U, assert_case_equals, rel
from variants_util import make_variants

pytestmark = pytest.mark.gpu

MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
RHO = 2700.0
FOUR = ("plate16", "holes3k", "frontal3k", "two_fans")
STEPS = 64
CG_TOL = 1e-12
ARRAYS = ("u", "v", "a", "f", "iterations", "probe_u", "probe_v", "probe_a", "energies", "snapshots")


@functools.lru_cache(maxsize=None)
def setup(name, config, lumped=False):
    """(prob, K, M, free, omega_1, T1) of mesh `name` under `config`: computed once, shared, left unchanged."""
    prob = MESHES[name][0]()
    if config == "load":
        prob = meshgen.config_fixed_left_point_load(prob.mesh)
    K, M, free = modal_ref.matrices(prob, RHO, lumped)
    lam, _ = modal_ref.eigenpairs(K, M, free, 2)
    w1 = float(np.sqrt(lam[0]))
    return prob, K, M, free, w1, 2.0 * np.pi / w1


def parameters(which, w1):
    """the two parameter sets of the issue: (beta, gamma, alpha, eta)"""
    return (0.25, 0.5, 0.0, 0.0) if which == "undamped" else (0.3025, 0.6, 0.05 * w1, 0.02 / w1)


def amplitude_of(config, dt, T1, steps=STEPS):
    """(a) the point load with amplitude[n] = 1 + sin(2 pi n dt / (0.7 T1)); (b) the pull-right displacement applied suddenly"""
    return 1.0 + np.sin(2.0 * np.pi * np.arange(steps + 1) * dt / (0.7 * T1)) if config == "load" else None


@functools.lru_cache(maxsize=None)
def twin(name, config, which, lumped=False):
    prob, K, M, free, w1, T1 = setup(name, config, lumped)
    beta, gamma, alpha, eta = parameters(which, w1)
    dt = T1 / 200.0
    return ref.newmark(K, M, free, prob.u_in, prob.f_in, STEPS, dt, beta, gamma, alpha, eta, amplitude_of(config, dt, T1))


def every_step(c, prob, steps, dt, amplitude=None, u0=None, v0=None, **kw):
    """u, v, a (steps + 1, 2N) and f (steps + 1, 2N, row 0 not available: NaN) of `steps` steps run one at a time (u0, v0: the
    start of the first)"""
    n2 = 2 * prob.mesh.num_nodes
    amp = np.ones(steps + 1) if amplitude is None else amplitude
    out = {k: np.full((steps + 1, n2), np.nan) for k in ("u", "v", "a", "f")}
    iterations = []
    for n in range(steps):
        first = n == 0
        r = c.transient(prob if first else None, steps=1, dt=dt, density=RHO, amplitude=amp[n:n + 2], resume=not first,
                        probes=np.arange(n2) if first else (), cg_tol=CG_TOL, u0=u0 if first else None, v0=v0 if first else None, **kw)
        if first:
            out["u"][0], out["v"][0], out["a"][0] = r["probe_u"][0], r["probe_v"][0], r["probe_a"][0]
            iterations.append(int(r["iterations"][0]))
        for k in ("u", "v", "a", "f"):
            out[k][n + 1] = r[k]
        iterations.append(int(r["iterations"][1]))
        assert r["converged"] == 1
    out["iterations"] = np.array(iterations)
    return out


def check_against_the_twin(out, want, what, rows=slice(None)):
    """the bars at every step; returns the worst figures"""
    worst = {}
    for k, tol in (("u", TOL_U), ("v", TOL_F), ("a", TOL_F), ("f", TOL_F)):
        errs = [rel(out[k][n], want[k][n]) for n in range(len(want[k]))[rows] if not np.isnan(out[k][n]).any() and np.any(want[k][n] != 0.0)]
        worst[k] = max(errs)
    print(what, "worst over the steps", worst, "iterations", int(out["iterations"].min()), "-", int(out["iterations"].max()))
    for k, tol in (("u", TOL_U), ("v", TOL_F), ("a", TOL_F), ("f", TOL_F)):
        assert worst[k] <= tol, (what, k, worst[k])
    return worst


def csr_entries(M, rowptr, col):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return np.asarray(M.tocsr()[rows, col]).reshape(-1)


@pytest.mark.parametrize("name", FOUR + ("clockwise",))
def test_assemble_effective_entry_by_entry(built, name):
    prob = meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24))) if name == "clockwise" else MESHES[name][0]()
    with Context(device=0) as c:
        c.upload_problem(prob)
        rowptr, col, K_dev = c.assemble_csr()
        got = {(lumped, cs): c.assemble_effective(cs[0], cs[1], RHO, lumped)
               for lumped in (False, True) for cs in ((1.0, 0.0), (0.0, 1.0), (0.37, 2.5e4))}
        assert np.array_equal(c.assemble_csr()[2], K_dev)  # (kval is not touched)
    for lumped in (False, True):
        M_ref = csr_entries(modal_ref.mass(prob.mesh.xy, prob.mesh.conn, RHO, prob.part_thickness, lumped), rowptr, col)
        if not lumped:
            assert np.count_nonzero(M_ref) > len(rowptr)  # (the consistent mass fills the pattern's blocks)
        for (c_K, c_M) in ((1.0, 0.0), (0.0, 1.0), (0.37, 2.5e4)):
            want = c_K * K_dev + c_M * M_ref
            err = float(np.max(np.abs(got[lumped, (c_K, c_M)] - want)) / np.max(np.abs(want)))
            print(name, "lumped" if lumped else "consistent", (c_K, c_M), "error / largest entry", err)
            assert err <= 1e-14
        assert np.array_equal(got[lumped, (1.0, 0.0)], K_dev)


@pytest.mark.parametrize("name", FOUR)
@pytest.mark.parametrize("mode", [1, 3])
def test_free_vibration_against_the_closed_form(built, name, mode):
    prob, K, M, free, lam, Phi = modal_ref.cached(name, RHO)
    n2 = 2 * prob.mesh.num_nodes
    k = mode - 1
    dt = 2.0 * np.pi / np.sqrt(lam[0]) / 200.0
    with Context(device=0) as c:  # (the supports at rest, no load: the uploaded values replaced by zeros)
        c.upload(prob.xy_flat, prob.conn_flat, prob.u_known, np.zeros(n2), np.zeros(n2), prob.youngs_modulus, prob.poisson_ratio,
                 prob.part_thickness)
        out = c.transient(steps=STEPS, dt=dt, density=RHO, u0=Phi[k], snapshot_every=1, cg_tol=CG_TOL)
    want = ref.mode_closed_form(lam[k], Phi[k], STEPS, dt)
    err = rel(out["snapshots"], want)
    print(name, "mode", mode, "u over all steps against the closed form", err, "iterations", out["iterations"].max())
    assert out["converged"] == 1 and out["snapshots"].shape == want.shape
    assert err <= TOL_U


@pytest.mark.parametrize("name", FOUR)
@pytest.mark.parametrize("config", ["load", "pull"])
@pytest.mark.parametrize("which", ["undamped", "damped"])
@pytest.mark.parametrize("cg", [1, 2, 3, 4])
def test_forced_response_against_the_twin(built, name, config, which, cg):
    prob, K, M, free, w1, T1 = setup(name, config)
    beta, gamma, alpha, eta = parameters(which, w1)
    dt = T1 / 200.0
    with Context(device=0) as c:
        out = every_step(c, prob, STEPS, dt, amplitude_of(config, dt, T1), beta=beta, gamma=gamma, rayleigh=(alpha, eta), cg=cg)
        info = c.transient_info()
    assert (info["cg_kernel"], info["preconditioner"]) == ((5, cg - 1) if cg <= 3 else (3, 0))
    check_against_the_twin(out, twin(name, config, which), (name, config, which, cg))


def test_forced_response_with_the_lumped_mass(built):
    prob, K, M, free, w1, T1 = setup("holes3k", "load", True)
    dt = T1 / 200.0
    with Context(device=0) as c:
        out = every_step(c, prob, STEPS, dt, amplitude_of("load", dt, T1), lumped=True)
    check_against_the_twin(out, twin("holes3k", "load", "undamped", True), "lumped")


@pytest.mark.parametrize("name", FOUR)
def test_energies(built, name):
    prob, K, M, free, w1, T1 = setup(name, "load")
    dt = T1 / 200.0
    with Context(device=0) as c:
        out = c.transient(prob, steps=STEPS, dt=dt, density=RHO, energies=True, cg_tol=CG_TOL)
    want = ref.newmark(K, M, free, prob.u_in, prob.f_in, STEPS, dt)
    T, W, P = out["energies"].T
    balance = T + W - P
    drift = float(np.max(np.abs(balance - balance[0])) / W.max())
    err = rel(W, want["energies"][:, 1])
    print(name, "drift of T + W - P / peak strain energy", drift, "W against the twin", err)
    assert W.max() > 0 and drift <= 1e-8
    assert err <= TOL_F


@pytest.mark.parametrize("cg", [0, 1, 2, 3, 4])
def test_records(built, cg):
    prob, K, M, free, w1, T1 = setup("holes3k", "load")
    dt = T1 / 200.0
    known = np.asarray(prob.u_known) != 0
    loaded = int(np.flatnonzero(np.asarray(prob.f_in) != 0)[0])
    probes = [int(np.flatnonzero(~known & (np.asarray(prob.f_in) == 0))[7]), int(np.flatnonzero(known)[3]), loaded]
    with Context(device=0) as c:
        out = c.transient(prob, steps=STEPS, dt=dt, density=RHO, probes=probes, snapshot_every=4, cg=cg, cg_tol=CG_TOL)
    assert out["snapshots"].shape == (STEPS // 4 + 1, 2 * prob.mesh.num_nodes)
    assert np.array_equal(out["probe_u"][::4], out["snapshots"][:, probes])  # bit for bit at the steps both hold
    assert np.array_equal(out["snapshots"][-1], out["u"])
    for k in ("u", "v", "a"):
        assert np.array_equal(out["probe_" + k][-1], out[k][probes]), k
    assert not out["probe_u"][:, 1].any() and not out["probe_v"][:, 1].any() and not out["probe_a"][:, 1].any()  # the support
    assert out["probe_a"][0, 2] > 0  # the load acts from t = 0
    assert out["iterations"].shape == (STEPS + 1,) and out["iterations"][0] > 0 and np.all(out["iterations"][1:] > 0)
    assert (out["t_start"], out["t_end"]) == (0.0, STEPS * dt)
    assert out["steps"] == STEPS and out["snapshots_kept"] == STEPS // 4 + 1 and out["resumed"] == 0 and out["converged"] == 1
    assert (out["cg_kernel"], out["preconditioner"]) == {0: (5, 2), 1: (5, 0), 2: (5, 1), 3: (5, 2), 4: (3, 0)}[cg]
    assert out["cg_iterations"] == int(out["iterations"].sum()) and out["max_step_iterations"] == int(out["iterations"].max())


@pytest.mark.parametrize("cg", [0, 4])
def test_zero_stays_zero(built, cg):
    prob, K, M, free, w1, T1 = setup("holes3k", "load")
    n2 = 2 * prob.mesh.num_nodes
    amp = np.ones(STEPS + 1)
    amp[:4] = 0.0
    with Context(device=0) as c:
        out = c.transient(prob, steps=STEPS, dt=T1 / 200.0, density=RHO, amplitude=amp, probes=np.arange(n2), cg=cg, cg_tol=CG_TOL)
    for k in ("probe_u", "probe_v", "probe_a"):
        assert not out[k][:4].any(), k
        assert not np.signbit(out[k][:4]).any(), k
    assert out["iterations"][:4].tolist() == [0, 0, 0, 0] and out["iterations"][4] > 0
    assert out["probe_a"][4].any() and out["converged"] == 1


def assert_same_bits(a, b, what):
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in Context.TRANSIENT_INFO + ("t_start", "t_end"):
        assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.mark.parametrize("cg", [0, 4])
def test_repeat_and_resume(built, cg):
    prob, K, M, free, w1, T1 = setup("holes3k", "load")
    n2 = 2 * prob.mesh.num_nodes
    dt = T1 / 200.0
    beta, gamma, alpha, eta = parameters("damped", w1)
    amp = amplitude_of("load", dt, T1)
    kw = dict(dt=dt, density=RHO, beta=beta, gamma=gamma, rayleigh=(alpha, eta), probes=np.arange(n2), energies=True, snapshot_every=4,
              cg=cg, cg_tol=CG_TOL)
    with Context(device=0) as c:
        whole = c.transient(prob, steps=STEPS, amplitude=amp, **kw)
        again = c.transient(steps=STEPS, amplitude=amp, **kw)
        head = c.transient(steps=24, amplitude=amp[:25], **kw)
        tail = c.transient(steps=40, amplitude=amp[24:], resume=True, **kw)
    with Context(device=0) as fresh:
        other = fresh.transient(prob, steps=STEPS, amplitude=amp, **kw)
    assert_same_bits(whole, again, "the same context")
    assert_same_bits(whole, other, "a fresh context")
    for k in ("probe_u", "probe_v", "probe_a", "energies"):
        assert np.array_equal(head[k], whole[k][:25]), k
        assert np.array_equal(tail[k], whole[k][24:]), k
    assert np.array_equal(head["snapshots"], whole["snapshots"][:7]) and np.array_equal(tail["snapshots"], whole["snapshots"][6:])
    assert np.array_equal(head["iterations"], whole["iterations"][:25])
    assert tail["iterations"][0] == 0 and np.array_equal(tail["iterations"][1:], whole["iterations"][25:])
    for k in ("u", "v", "a", "f"):
        assert np.array_equal(tail[k], whole[k]), k
    assert tail["resumed"] == 1 and head["resumed"] == 0
    assert (head["t_start"], head["t_end"]) == (0.0, 24 * dt) and tail["t_start"] == head["t_end"] and tail["t_end"] == head["t_end"] + 40 * dt


def test_fall_back_without_tile_local_tables(built):
    prob, K, M, free, w1, T1 = setup("holes3k", "load")
    dt = T1 / 200.0
    with Context(device=0, op_variant=1) as c:
        out = every_step(c, prob, STEPS, dt, amplitude_of("load", dt, T1), cg=0)
        info = c.transient_info()
        with pytest.raises(MagnetiteError) as e:
            c.transient(steps=2, dt=dt, density=RHO, cg=3)
        assert e.value.code == MAG_ERR_STATE and "tile-local" in e.value.message
    assert (info["cg_kernel"], info["preconditioner"]) == (3, 0)
    check_against_the_twin(out, twin("holes3k", "load", "undamped"), "op_variant 1")


def same(a, b, what):
    """dicts of arrays and numbers, bit for bit"""
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k)


def test_it_leaves_everything_else_alone(built):
    prob = MESHES["holes3k"][0]()
    V = 3
    xy, mat, u, f = make_variants(prob, V, seed=4)
    w = np.random.default_rng(8).uniform(0.5, 1.5, (V, 2 * prob.mesh.num_nodes))
    T1 = setup("holes3k", "pull")[5]
    scale = np.random.default_rng(3).uniform(0.5, 1.5, prob.mesh.num_elements)
    MODAL = ("lambda", "frequency", "residual", "shapes")

    def no_times(st):
        return {k: v for k, v in st.items() if not k.startswith("ms_")}

    def everything(c):
        out = dict(run=c.download(), stats=no_times(c.stats()), history=c.history(5), run_stress=c.download_stress("run", 0),
                   run_sens=c.download_sensitivity("run", 0), modal=c.download_modal(), modal_info=c.modal_info())
        for i in range(V):
            out[i] = dict(variant=c.download_variant(i), variant_stats=no_times(c.variant_stats(i)), case=c.download_case(i),
                          case_stats=no_times(c.case_stats(i)), sens=c.download_sensitivity("variants", i),
                          adjoint=c.download_adjoint("cases", i), adjoint_stats=no_times(c.adjoint_stats("cases", i)),
                          objective=c.download_objective("cases", i, total=True), stress=c.download_stress("variants", i))
        return out

    def compare(a, b):
        for x, y in zip(a["run"], b["run"]):
            assert np.array_equal(x, y)
        assert a["stats"] == b["stats"] and np.array_equal(a["history"], b["history"])
        same(a["run_stress"], b["run_stress"], "stress of the run")
        same(a["run_sens"], b["run_sens"], "sensitivities of the run")
        same(a["modal"], b["modal"], "the modes")
        assert a["modal_info"] == b["modal_info"]
        for i in range(V):
            for key in ("variant", "case"):
                for x, y in zip(a[i][key], b[i][key]):
                    assert np.array_equal(x, y), (i, key)
            for key in ("variant_stats", "case_stats", "adjoint_stats"):
                assert a[i][key] == b[i][key], (i, key)
            for key in ("sens", "adjoint", "objective", "stress"):
                same(a[i][key], b[i][key], (i, key))

    def field_run(c):
        c.set_element_scale(scale)
        c.run()
        return dict(zip(("u", "f", "stress"), c.download()), **c.stats())

    with Context(device=0, history_len=16, field_cg=3) as c:
        c.solve_variants(prob, xy, mat, u, f)
        c.set_load_cases(u, f)
        c.run_cases()
        c.run()
        c.run_sensitivities("variants")
        c.run_sensitivities("run")
        c.run_objective("disp_lsq", "cases", weights=w, adjoint=True)
        c.run_stress("variants")
        c.run_stress("run")
        c.run_modal(modes=4, density=RHO)
        before = everything(c)
        opts = {k: getattr(c.options, k) for k, _ in type(c.options)._fields_}
        for cg in (0, 4):
            out = c.transient(steps=16, dt=T1 / 200.0, density=RHO, cg=cg, energies=True, probes=[5], snapshot_every=2)
            assert out["converged"] == 1
            compare(before, everything(c))
            assert opts == {k: getattr(c.options, k) for k, _ in type(c.options)._fields_}
        # the pass's results survive the other entry points; a run afterwards is the run of a context that never saw it
        c.run()
        after_run = dict(zip(("u", "f", "stress"), c.download()), **c.stats())
        c.run_cases()
        kept = c.download_transient()
        for k in ARRAYS:
            assert np.array_equal(kept[k], out[k]), k
        after_field = field_run(c)
        c.upload_problem(prob)  # a new upload drops them
        for call in (c.download_transient, c.transient_info, lambda: c.run_transient(4, T1 / 200.0, RHO, resume=True)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE
    with Context(device=0, history_len=16, field_cg=3) as plain:
        assert_case_equals(plain.solve(prob), after_run, "a solve that never saw the transient pass")
        assert_case_equals(field_run(plain), after_field, "a run under a field that never saw the transient pass")
        assert after_field["cg_kernel"] == 5


def test_refusals_on_the_device(built):
    with Context(device=0) as c:
        c.upload_problem(meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24))))
        with pytest.raises(MagnetiteError) as e:
            c.run_transient(4, 1e-6, RHO)
        assert e.value.code == MAG_ERR_BAD_ARGS and "mag_run_transient" in e.value.message and "element 0 " in e.value.message
        prob = MESHES["plate16"][0]()
        n2 = 2 * prob.mesh.num_nodes
        c.upload_problem(prob)
        for probes, at in (([0, n2 - 1, n2], 2), ([-1, 3], 0)):
            with pytest.raises(MagnetiteError) as e:
                c.run_transient(4, 1e-6, RHO, probes=probes)
            assert e.value.code == MAG_ERR_BAD_ARGS and f"probes[{at}]" in e.value.message
        out = c.transient(steps=4, dt=1e-6, density=RHO, probes=[0, n2 - 1])
        assert out["probe_u"].shape == (5, 2)
        for call in (c.download_transient, c.transient_info):  # (a refused run leaves no results ...)
            call()
        with pytest.raises(MagnetiteError):
            c.run_transient(4, 1e-6, RHO, probes=[n2])
        with pytest.raises(MagnetiteError) as e:  # (... of the pass)
            c.download_transient()
        assert e.value.code == MAG_ERR_STATE
        c.set_element_scale(np.full(prob.mesh.num_elements, 0.5))
        for call in (lambda: c.run_transient(4, 1e-6, RHO), lambda: c.assemble_effective(1.0, 1.0, RHO)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE and "element stiffness field" in e.value.message
