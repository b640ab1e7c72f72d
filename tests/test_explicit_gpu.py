"""GPU: mag_run_explicit -- central differences on the lumped mass, one fused launch a step -- against the numpy twin of
tests/explicit_ref.py, the closed form of a lumped-mass mode and the implicit pass at beta = 0; the bound of the stable step;
every tile size and grid, records, repeats, resumed runs and device buffers bit for bit; the unfused fall-back; the hand-off
between the two passes; nothing else of the context changes; the refusals that need the device.

Cases (tests/explicit_cases.py): plate16, holes3k, frontal3k, two_fans of tests/test_load_cases_gpu.py as uploaded ("pull") and
under config_fixed_left_point_load ("load", amplitude[n] = 1 + sin(2 pi n dt / (0.7 T1))), one plate(4) on rollers; undamped
and the project's damped set (alpha = 0.05 w1, eta = 0.02 / w1).  256 steps at the device's own 0.9 dt_bound.

Bars (from the issue): relative L2 at every row, u 1e-10; v, a, the energies and the final reactions 1e-9 -- the twin against
itself under a random renumbering differs by 4.7e-15 / 2.2e-13 / 6.8e-13 (u / v / a), so the bars stand two to four orders
above rounding and two orders inside the project's parity bars.  The bound 1e-14; the closed form 1e-10; the implicit pass and
the hand-off TOL_U / TOL_F.

Measured on an MI355X, at worst over the 18 cases (fused | unfused): u 1.9e-13 | 1.9e-13, v 2.3e-13 | 2.3e-13,
a 9.9e-13 | 1.9e-12, the energies 4.5e-14 | 4.8e-14, the final reactions 1.6e-13 | 1.5e-13; the bound 4.6e-16; the closed form
1.4e-13; against the implicit pass u 9.3e-16, v 5.9e-15, a 2.2e-14, reactions 1.3e-13; the hand-off u 9.0e-16, a 2.9e-14."""
import ctypes as C

import numpy as np
import pytest

import explicit_cases as cases
import explicit_ref as ref
import modal_ref
from device_buffers import HostBuffer, Leg
from magnetite_amd import Context, _lib, meshgen
from magnetite_amd._lib import MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK
from magnetite_amd.solver import MagnetiteError
from test_load_cases_gpu import TOL_F, TOL_U, rel

pytestmark = pytest.mark.gpu

MAG_ERR_BAD_ARGS, MAG_ERR_STATE, MAG_ERR_NOT_CONVERGED = 1, 7, 3
RHO = cases.RHO
STEPS = 256
ARRAYS = ("u", "v", "a", "f", "iterations", "probe_u", "probe_v", "probe_a", "energies", "snapshots", "time")
WORST = {}


def same_bits(a, b, what, keys=ARRAYS):
    for k in keys:
        assert (k in a) == (k in b), (what, k)
        if k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def run_against_the_twin(name, config, which, what, **context):
    """256 steps at the device's own 0.9 dt_bound with probes at every DOF and the energies, against the twin at that dt"""
    prob, K, M, m, free, w1, T1 = cases.setup(name, config)
    alpha, eta = cases.rayleigh(which, w1)
    n2 = 2 * prob.mesh.num_nodes
    with Context(device=0, **context) as c:
        c.upload_problem(prob)
        dt = 0.9 * c.explicit_dt(RHO, eta)["dt_bound"]
        amp = cases.amplitude_of(config, dt, T1, STEPS)
        out = c.explicit(steps=STEPS, density=RHO, rayleigh=(alpha, eta), amplitude=amp, probes=np.arange(n2), energies=True)
    assert out["dt"] == dt and out["probe_u"].shape == (STEPS + 1, n2)
    want = ref.explicit(K, M, free, prob.u_in, prob.f_in, STEPS, dt, alpha, eta, amp)
    worst = {}
    for k, tol in (("u", 1e-10), ("v", 1e-9), ("a", 1e-9), ("energies", 1e-9)):
        got = out["energies"] if k == "energies" else out["probe_" + k]
        worst[k] = max([rel(got[n], want[k][n]) for n in range(STEPS + 1) if np.any(want[k][n] != 0.0)], default=0.0)
    worst["f"] = rel(out["f"], want["f"][STEPS])
    for k in ("u", "v", "a"):
        assert np.array_equal(out[k], out["probe_" + k][STEPS]), k
    print(what, name, config, which, "worst over the rows", worst)
    for k, w in worst.items():
        WORST[what, k] = max(WORST.get((what, k), 0.0), w)
    print(what, "worst so far", {k: v for (w, k), v in WORST.items() if w == what})
    for k, tol in (("u", 1e-10), ("v", 1e-9), ("a", 1e-9), ("energies", 1e-9), ("f", 1e-9)):
        assert worst[k] <= tol, (what, name, config, which, k, worst[k])
    return out


# ---- 1. parity with the twin
@pytest.mark.parametrize("name, config", cases.CASES)
@pytest.mark.parametrize("which", ["undamped", "damped"])
def test_parity_with_the_twin(built, name, config, which):
    out = run_against_the_twin(name, config, which, "fused")
    assert (out["method"], out["fused"], out["step_launches"], out["record_every"], out["finite"]) == (6, 1, STEPS + 1, 1, 1)
    assert not out["iterations"].any() and len(out["iterations"]) == STEPS + 1


# ---- 2. the bound
@pytest.mark.parametrize("name, config", cases.CASES)
def test_the_bound_against_the_twin(built, name, config):
    prob, K, M, m, free, w1, T1 = cases.setup(name, config)
    eta = 0.02 / w1
    with Context(device=0) as c:
        c.upload_problem(prob)
        got = c.explicit_dt(RHO, eta)
        out = c.explicit(steps=2, density=RHO, rayleigh=(0.0, eta))
        scaled = c.explicit(steps=2, density=RHO, rayleigh=(0.0, eta), dt_scale=0.5)
        given = c.explicit(steps=2, density=RHO, rayleigh=(0.0, eta), dt=1e-9)
    want = dict(lambda_bound=ref.lambda_bound(K, m, free), dt_bound_undamped=ref.bound(K, m, free), dt_bound=ref.bound(K, m, free, eta),
                min_mass=float(m.min()))
    errs = {k: abs(got[k] - want[k]) / want[k] for k in want}
    print(name, config, "the bound against the twin", errs)
    assert max(errs.values()) <= 1e-14
    assert out["dt_bound"] == got["dt_bound"] == scaled["dt_bound"] == given["dt_bound"]
    assert out["dt"] == 0.9 * got["dt_bound"] and scaled["dt"] == 0.5 * got["dt_bound"] and given["dt"] == 1e-9
    assert out["t_end"] == 2 * out["dt"] and np.array_equal(out["time"], out["dt"] * np.arange(3))


# ---- 3. the closed form
@pytest.mark.parametrize("name", ["plate16", "holes3k"])
@pytest.mark.parametrize("mode", [1, 2])
def test_free_vibration_against_the_closed_form(built, name, mode):
    prob, K, M, free, lam, Phi = modal_ref.cached(name, RHO, True)
    n2 = 2 * prob.mesh.num_nodes
    k = mode - 1
    with Context(device=0) as c:  # (the supports at rest, no load: the uploaded values replaced by zeros)
        c.upload(prob.xy_flat, prob.conn_flat, prob.u_known, np.zeros(n2), np.zeros(n2), prob.youngs_modulus, prob.poisson_ratio,
                 prob.part_thickness)
        out = c.explicit(steps=64, density=RHO, u0=Phi[k], snapshot_every=1)
    want = ref.mode_closed_form(lam[k], Phi[k], 64, out["dt"])
    err = float(np.abs(out["snapshots"] - want).max() / np.abs(Phi[k]).max())
    print(name, "mode", mode, "u over all steps against the closed form", err, "relative L2", rel(out["snapshots"], want))
    assert out["snapshots"].shape == want.shape
    assert err <= 1e-10 and rel(out["snapshots"], want) <= 1e-10


# ---- 4. against the implicit pass
@pytest.mark.parametrize("name, config", [("plate16", "load"), ("holes3k", "pull"), ("two_fans", "load")])
@pytest.mark.parametrize("cg", [1, 4])
def test_against_the_implicit_pass_at_beta_zero(built, name, config, cg):
    prob, K, M, m, free, w1, T1 = cases.setup(name, config)
    n2 = 2 * prob.mesh.num_nodes
    alpha = 0.05 * w1
    with Context(device=0) as c:
        c.upload_problem(prob)
        dt = 0.9 * c.explicit_dt(RHO)["dt_bound"]
        amp = cases.amplitude_of(config, dt, T1, 32)
        kw = dict(steps=32, dt=dt, density=RHO, rayleigh=(alpha, 0.0), amplitude=amp, probes=np.arange(n2))
        ex = c.explicit(**kw)
        im = c.transient(beta=0.0, gamma=0.5, lumped=True, cg=cg, cg_tol=1e-14, **kw)
    assert im["converged"] == 1 and im["cg_kernel"] == (5 if cg == 1 else 3)
    worst = {}
    for k, tol in (("u", TOL_U), ("v", TOL_F), ("a", TOL_F)):
        worst[k] = max(rel(ex["probe_" + k][n], im["probe_" + k][n]) for n in range(33) if np.any(im["probe_" + k][n] != 0.0))
        assert worst[k] <= tol, (k, worst[k])
    worst["f"] = rel(ex["f"], im["f"])
    print(name, config, "cg", cg, "explicit against the implicit pass", worst)
    assert worst["f"] <= TOL_F


# ---- 5. every tile size and grid: the same bits
@pytest.mark.parametrize("name", ["holes3k", "two_fans"])
def test_every_tile_size_and_grid_gives_the_same_bits(built, name, monkeypatch):
    prob, K, M, m, free, w1, T1 = cases.setup(name, "load")
    alpha, eta = cases.rayleigh("damped", w1)
    n2 = 2 * prob.mesh.num_nodes
    runs = {}
    for tile in (256, 512, 1024):
        for grid in ("1", "2", None):
            if grid is None:
                monkeypatch.delenv("MAG_TUNE_GRID", raising=False)
            else:
                monkeypatch.setenv("MAG_TUNE_GRID", grid)
            with Context(device=0, tile_nodes=tile) as c:
                c.upload_problem(prob)
                runs[tile, grid] = c.explicit(steps=48, density=RHO, rayleigh=(alpha, eta), probes=np.arange(n2), energies=True,
                                              snapshot_every=16, amplitude=cases.amplitude_of("load", 1e-6, T1, 48))
            assert runs[tile, grid]["fused"] == 1, (tile, grid)
    first = runs[256, "1"]
    assert np.abs(first["u"]).max() > 0
    for key, out in runs.items():
        same_bits(out, first, (name, key))
        assert out["dt"] == first["dt"] and out["dt_bound"] == first["dt_bound"]


# ---- 6. the unfused fall-back
@pytest.mark.parametrize("name, config", cases.CASES)
@pytest.mark.parametrize("which", ["undamped", "damped"])
def test_the_unfused_fall_back(built, name, config, which):
    out = run_against_the_twin(name, config, which, "unfused", op_variant=1)
    assert (out["method"], out["fused"], out["step_launches"]) == (6, 0, 4 * (STEPS + 1))


# ---- 7. records
@pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["fused", "unfused"])
def test_records(built, context):
    prob, K, M, m, free, w1, T1 = cases.setup("holes3k", "pull")
    alpha, eta = cases.rayleigh("damped", w1)
    n2 = 2 * prob.mesh.num_nodes
    known = np.asarray(prob.u_known) != 0
    steps = 44
    runs = {}
    with Context(device=0, **context) as c:
        c.upload_problem(prob)
        for re in (1, 3, 7):
            for se in (0, 5):
                runs[re, se] = c.explicit(steps=steps, density=RHO, rayleigh=(alpha, eta), probes=np.arange(n2), energies=True,
                                          record_every=re, snapshot_every=se)
    every = runs[1, 5]
    assert np.any(np.asarray(prob.u_in)[known] != 0.0)
    for (re, se), out in runs.items():
        rows = steps // re + 1
        same_bits(out, every, (re, se), ("u", "v", "a", "f"))
        assert out["record_every"] == re and out["step_launches"] == (steps + 1) * (1 if not context else 4)
        assert out["probe_u"].shape == (rows, n2) and out["energies"].shape == (rows, 3) and out["iterations"].shape == (rows,)
        for k in ("probe_u", "probe_v", "probe_a", "energies"):
            assert out[k].tobytes() == every[k][::re].tobytes(), (re, se, k)
        assert np.array_equal(out["time"], every["time"][::re])
        if se:
            assert out["snapshots_kept"] == steps // se + 1 and out["snapshots"].tobytes() == every["probe_u"][::se].tobytes(), (re, se)
        else:
            assert out["snapshots_kept"] == 0 and "snapshots" not in out
        # the supports: u_in's bits and zero v, a in every row
        assert np.array_equal(out["probe_u"][:, known], np.broadcast_to(np.asarray(prob.u_in)[known], (rows, int(known.sum()))))
        assert not out["probe_v"][:, known].any() and not out["probe_a"][:, known].any()


# ---- 8. repeat and resume
@pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["fused", "unfused"])
def test_repeat_and_resume(built, context):
    prob, K, M, m, free, w1, T1 = cases.setup("holes3k", "load")
    alpha, eta = cases.rayleigh("damped", w1)
    n2 = 2 * prob.mesh.num_nodes
    n1, n2_steps = 21, 27
    with Context(device=0, **context) as c:
        c.upload_problem(prob)
        dt = 0.9 * c.explicit_dt(RHO, eta)["dt_bound"]
        amp = cases.amplitude_of("load", dt, T1, n1 + n2_steps)
        kw = dict(density=RHO, rayleigh=(alpha, eta), probes=np.arange(n2), energies=True)
        whole = c.explicit(steps=n1 + n2_steps, amplitude=amp, snapshot_every=3, **kw)
        again = c.explicit(steps=n1 + n2_steps, amplitude=amp, snapshot_every=3, **kw)
        first = c.explicit(steps=n1, amplitude=amp[:n1 + 1], snapshot_every=3, **kw)
        resumed_amp = amp[n1:].copy()
        resumed_amp[0] = np.nan  # (ignored: row 0 carries the load of the state it resumes)
        second = c.explicit(steps=n2_steps, amplitude=resumed_amp, snapshot_every=3, resume=True, **kw)
        c.explicit(steps=n1, amplitude=amp[:n1 + 1], **kw)
        thirds = c.explicit(steps=n2_steps, amplitude=resumed_amp, record_every=3, resume=True, **kw)
    same_bits(again, whole, "repeat")
    assert (first["resumed"], second["resumed"], second["step_launches"]) == (0, 1, n2_steps * (1 if not context else 4))
    assert second["t_start"] == first["t_end"] and second["t_end"] == first["t_end"] + n2_steps * dt
    same_bits(second, whole, "resumed", ("u", "v", "a", "f"))
    for k in ("probe_u", "probe_v", "probe_a", "energies"):
        assert first[k].tobytes() == whole[k][:n1 + 1].tobytes(), k
        assert second[k].tobytes() == whole[k][n1:].tobytes(), k
        assert thirds[k].tobytes() == whole[k][n1::3].tobytes(), k
    assert second["snapshots"].tobytes() == whole["snapshots"][n1 // 3:].tobytes()
    same_bits(thirds, whole, "resumed under another record_every", ("u", "v", "a", "f"))


@pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["fused", "unfused"])
def test_a_zero_state_stays_zero(built, context):
    prob = cases.setup("holes3k", "load")[0]
    n2 = 2 * prob.mesh.num_nodes
    with Context(device=0, **context) as c:
        c.upload(prob.xy_flat, prob.conn_flat, prob.u_known, np.zeros(n2), np.zeros(n2), prob.youngs_modulus, prob.poisson_ratio,
                 prob.part_thickness)
        out = c.explicit(steps=16, density=RHO, rayleigh=(3.0, 1e-7), probes=np.arange(n2), energies=True, snapshot_every=4)
    for k in ("u", "v", "a", "f", "probe_u", "probe_v", "probe_a", "energies", "snapshots"):
        assert not out[k].any(), k


# ---- 9. the hand-off between the passes
@pytest.mark.parametrize("order", ["explicit first", "implicit first"])
def test_hand_off_between_the_passes(built, order):
    prob, K, M, m, free, w1, T1 = cases.setup("holes3k", "load")
    alpha = 0.05 * w1
    with Context(device=0) as c:
        c.upload_problem(prob)
        dt = 0.9 * c.explicit_dt(RHO)["dt_bound"]
        amp = cases.amplitude_of("load", dt, T1, 40)
        ex = dict(dt=dt, density=RHO, rayleigh=(alpha, 0.0))
        im = dict(ex, beta=0.0, gamma=0.5, lumped=True, cg_tol=1e-14)
        whole = c.explicit(steps=40, amplitude=amp, **ex)
        if order == "explicit first":
            c.explicit(steps=20, amplitude=amp[:21], **ex)
            out = c.transient(steps=20, amplitude=amp[20:], resume=True, **im)
            assert (out["cg_kernel"], out["resumed"], out["converged"]) == (5, 1, 1)
        else:
            c.transient(steps=20, amplitude=amp[:21], **im)
            out = c.explicit(steps=20, amplitude=amp[20:], resume=True, **ex)
            assert (out["method"], out["resumed"]) == (6, 1)
    worst = {k: rel(out[k], whole[k]) for k in ("u", "v", "a", "f")}
    print(order, "against 40 explicit steps", worst)
    assert out["t_start"] == 20 * dt and abs(out["t_end"] - whole["t_end"]) <= 1e-15 * whole["t_end"]
    assert worst["u"] <= TOL_U and max(worst["v"], worst["a"], worst["f"]) <= TOL_F


# ---- 10. device buffers
class ExplicitLeg(Leg):
    def run_explicit(self, steps, density, amplitude=None, u0=None, v0=None, probes=None, **options):
        """Leg.run_transient's treatment of the inputs, for mag_run_explicit"""
        ins = [self._in(amplitude), self._in(u0), self._in(v0)]
        p = None
        if probes is not None:
            p = np.ascontiguousarray(probes, dtype=np.int32)
            p = self.arena.put(p, 4 if self.offset else 0) if self.device else HostBuffer(p)
        o = _lib.ExplicitOptions()
        self.L.mag_default_explicit_options(C.byref(o))
        o.steps, o.density, o.memory = int(steps), float(density), self.memory
        o.amplitude, o.u0, o.v0, o.probes = (self._ptr(b) for b in ins + [p])
        o.num_probes = 0 if probes is None else len(probes)
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        rc = self.L.mag_run_explicit(self.h, C.byref(o))
        self._called(ins + [p], scribble=True, keep=True)
        self._transient = (o.num_probes, bool(o.energies))
        return rc


def test_the_explicit_pass_reads_and_writes_device_memory(built):
    from device_buffers import DeviceArena
    prob, K, M, m, free, w1, T1 = cases.setup("plate16", "load")
    alpha, eta = cases.rayleigh("damped", w1)
    n2 = 2 * prob.mesh.num_nodes
    lam, Phi = modal_ref.eigenpairs(K, M, free, 2)
    u0, v0 = 1e-4 * Phi[0], 1e-1 * Phi[1]
    probes = np.arange(n2 - 1, -1, -3)
    opts = dict(rayleigh_mass=alpha, rayleigh_stiffness=eta, energies=1, snapshot_every=3)
    out = {}
    with DeviceArena() as arena, Context(device=0) as host, Context(device=0) as dev:
        for key, leg in (("host", ExplicitLeg(host, MAG_MEM_HOST)), ("device", ExplicitLeg(dev, MAG_MEM_DEVICE, arena, 8))):
            leg.ctx.upload_problem(prob)
            dt = 0.9 * leg.ctx.explicit_dt(RHO, eta)["dt_bound"]
            amp = cases.amplitude_of("load", dt, T1, 15)
            resumed_amp = amp[10:].copy()
            resumed_amp[0] = np.nan
            assert leg.run_explicit(10, RHO, amp[:11], u0, v0, probes, **opts) == MAG_OK, leg.error()
            out[key, "first"] = leg.download_transient()
            assert leg.run_explicit(5, RHO, resumed_amp, probes=probes[:7], resume=1, **opts) == MAG_OK, leg.error()
            out[key, "resumed"] = leg.download_transient()
        arena.check()
    for part in ("first", "resumed"):
        got, want = out["device", part], out["host", part]
        assert list(got) == list(want)
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (part, k)
            if isinstance(got[k], np.ndarray) and got[k].dtype == np.float64:
                assert np.isfinite(got[k]).all() and (k == "energies" or np.any(got[k] != 0.0)), (part, k)
    assert out["device", "first"]["probe_u"].shape == (11, len(probes)) and out["device", "first"]["snapshots"].shape == (4, n2)
    assert out["device", "resumed"]["probe_u"].shape == (6, 7) and out["device", "resumed"]["snapshots"].shape == (2, n2)
    # the binding's own path, host memory throughout, on a third context
    with Context(device=0) as c:
        c.upload_problem(prob)
        dt = 0.9 * c.explicit_dt(RHO, eta)["dt_bound"]
        first = c.explicit(steps=10, density=RHO, rayleigh=(alpha, eta), amplitude=cases.amplitude_of("load", dt, T1, 15)[:11], u0=u0, v0=v0,
                           probes=probes, energies=True, snapshot_every=3)
    for k, a in out["device", "first"].items():
        assert np.asarray(a).tobytes() == np.asarray(first[k]).tobytes(), k


# ---- 11. leaves the rest alone
def test_the_other_results_keep_their_bits(built):
    from load_cases_util import make_cases
    prob = cases.setup("holes3k", "pull")[0]
    u, f = make_cases(prob, 3, seed=5)
    with Context(device=0) as c:
        def others():
            out = dict(zip(("u", "f", "stress"), c.download()))
            for i in range(3):
                out.update({(i, k): a for k, a in zip(("u", "f", "stress"), c.download_case(i))})
            out.update({("modal", k): a for k, a in c.download_modal().items()})
            return out
        c.upload_problem(prob)
        c.set_load_cases(u, f)
        c.run_cases()
        c.run()
        c.run_modal(3, RHO)
        before = others()
        out = c.explicit(steps=32, density=RHO, rayleigh=(1.0, 1e-7), probes=[0, 5], energies=True, snapshot_every=8)
        after = others()
        assert np.abs(out["v"]).max() > 0
    assert list(before) == list(after)
    for k in before:
        assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k


@pytest.mark.parametrize("what", ["field", "assemble_csr", "precision"])
def test_the_contexts_the_transient_pass_refuses(built, what):
    prob = cases.setup("plate16", "pull")[0]
    options = dict(assemble_csr=0) if what == "assemble_csr" else (dict(precision=1) if what == "precision" else {})
    word = dict(field="element stiffness field", assemble_csr="assemble_csr = 0", precision="precision = 1")[what]
    with Context(device=0, **options) as c:
        c.upload_problem(prob)
        if what == "field":
            c.set_element_scale(np.full(prob.mesh.num_elements, 0.5))
        seen = []
        for call in (lambda: c.explicit(steps=4, density=RHO), lambda: c.explicit_dt(RHO),
                     lambda: c.transient(steps=4, dt=1e-7, density=RHO)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE and word in str(e.value), str(e.value)
            seen.append(str(e.value).split(":", 2)[-1])
        assert seen[0] == seen[2]  # (the transient pass's wording)


# ---- 12. the refusals that need the device
def test_a_clockwise_element_and_a_probe_out_of_range_are_named(built):
    prob = cases.setup("plate16", "load")[0]
    n2 = 2 * prob.mesh.num_nodes
    conn = np.array(prob.mesh.conn, dtype=np.int32)
    conn[37] = conn[37][::-1]
    with Context(device=0) as c:
        c.upload(prob.xy_flat, conn.reshape(-1), prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus, prob.poisson_ratio,
                 prob.part_thickness)
        with pytest.raises(MagnetiteError) as e:
            c.explicit(steps=4, density=RHO)
        assert e.value.code == MAG_ERR_BAD_ARGS and "mag_run_explicit: element 37 has a signed area <= 0" in str(e.value)
        c.upload_problem(prob)
        for probes, k in (([0, n2], 1), ([3, 4, -1, n2], 2)):
            with pytest.raises(MagnetiteError) as e:
                c.explicit(steps=4, density=RHO, probes=probes)
            assert e.value.code == MAG_ERR_BAD_ARGS and f"mag_run_explicit: probes[{k}] is outside [0, {n2})" in str(e.value)
        with pytest.raises(MagnetiteError):
            c.download_transient()  # (a failure leaves no results of the pass)
        assert c.explicit(steps=4, density=RHO, probes=[0, n2 - 1])["finite"] == 1


@pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["fused", "unfused"])
def test_a_step_far_above_the_bound_overflows_and_is_reported(built, context):
    prob = meshgen.config_fixed_left_point_load(meshgen.plate(4))
    with Context(device=0, **context) as c:
        c.upload_problem(prob)
        bound = c.explicit_dt(RHO)["dt_bound"]
        good = c.explicit(steps=8, density=RHO)
        with pytest.raises(MagnetiteError) as e:
            c.explicit(steps=300, density=RHO, dt=100.0 * bound)
        msg = str(e.value)
        assert e.value.code == MAG_ERR_NOT_CONVERGED and "mag_run_explicit" in msg
        assert ("dt = %g" % (100.0 * bound)) in msg and ("dt_bound = %g" % bound) in msg
        with pytest.raises(MagnetiteError):
            c.download_transient()  # (the pass's results are gone)
        with pytest.raises(MagnetiteError):
            c.explicit(steps=4, density=RHO, resume=True)
        again = c.explicit(steps=8, density=RHO)  # (and the context is usable as before)
    same_bits(again, good, "after the overflow")
