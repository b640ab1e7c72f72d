"""GPU: mag_run_transient_tl and mag_assemble_effective_tangent against the numpy twin of tests/transient_tl_ref.py on the cases
of tests/transient_tl_cases.py: the effective tangent bit for bit, the runs of every case with and without tile-local tables,
every cg, both masses, an amplitude, a moving start, snapshots, the same bits (a repeat, a resumed run, the poll's block length),
resumes into and out of the linear pass, the iteration cap, no side effects, device buffers, refusals.

Bars (from the issue; the transient pass's, DESIGN.md TR): Newton iteration counts per step equal the twin's; the final u within
1e-8 of the twin run on to its round-off floor (extra = 3); v, a, the reactions on P, the probe rows and the energy rows within 1e-7;
the element rows within 1e-12 of the twin's at the device's own u; mag_assemble_effective_tangent the bits of
c_K * assemble_tangent(u) + c_M * M.  Settings: newton_tol 1e-10, cg_tol 1e-12.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import newton_ref as nr
import transient_tl_cases as cases
import transient_tl_ref as ref
from device_buffers import UNWRITTEN, DeviceArena, HostBuffer, Leg, _dp
from magnetite_amd import Context, MagnetiteError, _lib, meshgen
from magnetite_amd._lib import MAG_ERR_BAD_ARGS, MAG_ERR_STATE, MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK
from test_load_cases_gpu import MESHES

pytestmark = pytest.mark.gpu

RHO = cases.RHO
rel = cases.rel
SET = dict(newton_tol=cases.NEWTON_TOL, cg_tol=cases.CG_TOL)
CONTEXTS = pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["tables", "op_variant1"])


# ---- 1. the effective tangent, bit for bit
def effective_in_numpy(c, u, c_K, c_M, lumped):
    """effective_values's expression on assemble_tangent(u) and the mass: c_K k everywhere, + c_M m where a block's diagonal is"""
    rowptr, col, _ = c.assemble_csr()
    kt = c.assemble_tangent(u)
    m = c.assemble_effective(0.0, 1.0, RHO, lumped)  # (0 k + m on the blocks' diagonals)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    on = (row & 1) == (np.asarray(col) & 1)
    ck = c_K * kt
    return np.where(on, ck + c_M * m, ck)


@pytest.mark.parametrize("name", cases.FOUR)
@pytest.mark.parametrize("context", [{}, dict(op_variant=1), dict(tile_nodes=256)], ids=["tables", "op_variant1", "tile256"])
def test_the_effective_tangent_bit_for_bit(built, name, context):
    s = cases.setup(name, "load300")
    p, dt = s["prob"], s["dt"]
    u = cases.twin(name, "load300")["u"][-1]
    with Context(device=0, **context) as c:
        c.upload_problem(p)
        for what, w in (("u = 0", np.zeros_like(u)), ("the twin's final u", u)):
            for lumped, (c_K, c_M) in ((False, (0.25 * dt * dt, 1.0)), (True, (0.3 * dt * dt, 1.0 + 0.01))):
                got = c.assemble_effective_tangent(w, c_K, c_M, RHO, lumped)
                want = effective_in_numpy(c, w, c_K, c_M, lumped)
                again = c.assemble_effective_tangent(w, c_K, c_M, RHO, lumped)
                differ = int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
                print(name, context, what, "lumped" if lumped else "consistent", "entries", got.size, "entries of other bits", differ)
                assert differ == 0
                assert got.tobytes() == again.tobytes()
        assert np.abs(c.assemble_effective_tangent(u, 1.0, 0.0, RHO) - c.assemble_csr()[2]).max() > 0  # (the state matters)


# ---- 2. the runs
def step_sums(out):
    """the CG iterations of every step, from the per-iteration records"""
    end = np.concatenate([[0], np.cumsum(out["newton_iterations"])])
    return np.array([out["newton_cg"][a:b].sum() for a, b in zip(end[:-1], end[1:])])


def check_against_the_twin(p, out, want, floor, probes, what, amp_last=1.0):
    known = np.asarray(p.u_known).reshape(-1) != 0
    steps = len(want["newton_iterations"]) - 1
    print(what, "newton_iterations", out["newton_iterations"].tolist(), "the twin's", want["newton_iterations"].tolist(), "cg", out["iterations"].tolist())
    assert np.array_equal(out["newton_iterations"], want["newton_iterations"])
    assert out["steps"] == steps and out["converged"] == 1 and not out["inverted"] and out["max_step_newton"] == want["newton_iterations"].max()
    err = {k: rel(out[k], floor[k][-1]) for k in ("u", "v", "a")}
    err["f_P"] = rel(out["f"][known], floor["f"][-1][known])
    for k in ("u", "v", "a"):
        err["probe_" + k] = max(rel(out["probe_" + k][n], floor[k][n][probes]) for n in range(steps + 1))
    err["energies"] = max(rel(out["energies"][:, k], floor["energies"][:, k]) for k in range(3))
    rows = nr.element_rows(*nr.of_problem(p), out["u"])
    err["elements"] = (np.abs(out["elements"] - rows).max(axis=0) / np.abs(rows).max(axis=0)).max()
    print(what, " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert err["u"] <= 1e-8
    assert max(err[k] for k in ("v", "a", "f_P", "probe_u", "probe_v", "probe_a", "energies")) <= 1e-7
    assert err["elements"] <= 1e-12
    assert np.array_equal(out["f"][~known], (amp_last * np.asarray(p.f_in))[~known])
    assert np.array_equal(out["probe_u"][-1], out["u"][probes]) and np.array_equal(out["probe_a"][-1], out["a"][probes])
    assert len(out["newton_residuals"]) == len(out["newton_cg"]) == out["newton_iterations_total"] == out["newton_iterations"].sum()
    assert np.array_equal(step_sums(out)[1:], out["iterations"][1:]) and out["newton_cg"].sum() + out["iterations"][0] == out["cg_iterations_total"]
    early = want["residuals"] > 1e-8  # (the ratios above the floor's reach: the device's are the twin's)
    assert rel(out["newton_residuals"][early], want["residuals"][early]) <= 1e-4


def device_run(c, name, kind, lumped=False, **kw):
    s = cases.setup(name, kind, lumped)
    n2 = 2 * s["prob"].mesh.num_nodes
    probes = np.arange(n2)  # (every DOF: a probe row is measured like the final state, against the whole vector)
    out = c.transient(s["prob"], steps=s["steps"], dt=s["dt"], density=RHO, rayleigh=(s["alpha"], 0.0), u0=s["u0"], probes=probes, energies=True,
                      kinematics="tl", lumped=lumped, **SET, **kw)
    return s, probes, out


@pytest.mark.parametrize("name, kind", cases.CASES)
@CONTEXTS
def test_the_run_against_the_twin(built, name, kind, context):
    with Context(device=0, **context) as c:
        s, probes, out = device_run(c, name, kind)
    assert (out["cg_kernel"], out["preconditioner"]) == ((3, 0) if context else (5, 2))
    check_against_the_twin(s["prob"], out, cases.twin(name, kind), cases.twin(name, kind, extra=3), probes, (name, kind, context))
    assert out["t_start"] == 0.0 and out["t_end"] == s["steps"] * s["dt"]


@pytest.mark.parametrize("cg", [1, 2, 3, 4])
def test_every_cg_on_plate16(built, cg):
    with Context(device=0) as c:
        s, probes, out = device_run(c, "plate16", "load300", cg=cg)
    assert (out["cg_kernel"], out["preconditioner"]) == ((3, 0) if cg == 4 else (5, cg - 1))
    check_against_the_twin(s["prob"], out, cases.twin("plate16", "load300"), cases.twin("plate16", "load300", extra=3), probes, ("plate16", "cg", cg))


def test_the_lumped_mass(built):
    with Context(device=0) as c:
        s, probes, out = device_run(c, "plate16", "load300", lumped=True)
    want, floor = cases.twin("plate16", "load300", lumped=True), cases.twin("plate16", "load300", extra=3, lumped=True)
    check_against_the_twin(s["prob"], out, want, floor, probes, ("plate16", "lumped"))
    assert rel(out["u"], cases.twin("plate16", "load300", extra=3)["u"][-1]) > 1e-4  # (the mass matters)


def twin_of(s, extra, **kw):
    p = s["prob"]
    return ref.newmark_tl(*ref.of_problem(p), s["M"], s["free"], p.u_in, p.f_in, s["steps"], s["dt"], alpha=s["alpha"], newton_tol=cases.NEWTON_TOL,
                          extra=extra, **kw)


def test_an_amplitude_a_moving_start_and_snapshots(built):
    """amplitude, u0 and v0 given (the entries of u0 / v0 on P are ignored: NaN), damping, snapshots every 3 steps"""
    s = dict(cases.setup("plate16", "pull5d"))
    p = s["prob"]
    n2 = 2 * p.mesh.num_nodes
    known = np.asarray(p.u_known).reshape(-1) != 0
    amp = 1.0 + 0.5 * np.sin(np.arange(s["steps"] + 1))
    x = p.mesh.xy[:, 0] - p.mesh.xy[:, 0].min()
    v0 = np.zeros((n2 // 2, 2))
    v0[:, 1] = 40.0 * x
    u0, v0 = np.array(s["u0"]), v0.reshape(-1)
    kw = dict(amplitude=amp, u0=np.where(known, 0.0, u0), v0=np.where(known, 0.0, v0))
    want, floor = twin_of(s, 0, **kw), twin_of(s, 3, **kw)
    probes = np.arange(0, n2, 5)
    with Context(device=0) as c:
        out = c.transient(p, steps=s["steps"], dt=s["dt"], density=RHO, rayleigh=(s["alpha"], 0.0), amplitude=amp, u0=np.where(known, np.nan, u0),
                          v0=np.where(known, np.nan, v0), probes=probes, energies=True, snapshot_every=3, kinematics="tl", **SET)
    check_against_the_twin(p, out, want, floor, probes, ("plate16", "amplitude, u0, v0"), amp_last=amp[-1])
    assert out["snapshots"].shape == (s["steps"] // 3 + 1, n2) and out["snapshots_kept"] == s["steps"] // 3 + 1
    for k in range(out["snapshots"].shape[0]):
        err = rel(out["snapshots"][k], floor["u"][3 * k])
        print("snapshot", k, err)
        assert err <= 1e-7
    assert np.array_equal(out["probe_u"][::3], out["snapshots"][:, probes])
    assert np.array_equal(out["probe_v"][0], np.where(known, 0.0, v0)[probes])


# ---- 3. the same bits
def same_bits(a, b, what, skip=()):
    assert list(a) == list(b), what
    for k in a:
        if k not in skip:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def test_a_repeat_a_resumed_run_and_the_poll_give_the_same_bits(built):
    s = cases.setup("holes3k", "pull5d")
    p = s["prob"]
    kw = dict(dt=s["dt"], density=RHO, rayleigh=(s["alpha"], 0.0), probes=[0, 7, 11], energies=True, kinematics="tl", **SET)
    runs = {}
    for every in (2, 64, 4096):
        with Context(device=0, check_every=every) as c:
            c.upload_problem(p)
            runs[every] = c.transient(steps=8, u0=s["u0"], **kw)
            if every == 64:
                again = c.transient(steps=8, u0=s["u0"], **kw)
                first = c.transient(steps=3, u0=s["u0"], **kw)
                rest = c.transient(steps=5, resume=True, **kw)
    same_bits(again, runs[64], "repeat")
    for every in (2, 4096):
        same_bits(runs[every], runs[64], f"check_every {every} against 64")
    whole = runs[64]
    assert rest["t_start"] == first["t_end"] and rest["t_end"] == whole["t_end"] and rest["steps"] == 5
    for k in ("u", "v", "a", "f", "elements"):
        assert rest[k].tobytes() == whole[k].tobytes(), k
    for k in ("probe_u", "probe_v", "probe_a", "energies"):
        assert first[k].tobytes() == whole[k][:4].tobytes() and rest[k].tobytes() == whole[k][3:].tobytes(), k
    assert np.array_equal(first["newton_iterations"][1:], whole["newton_iterations"][1:4])
    assert np.array_equal(rest["newton_iterations"][1:], whole["newton_iterations"][4:]) and rest["iterations"][0] == 0


def test_resumes_into_and_out_of_the_linear_pass(built):
    """a linear run resumed as a nonlinear one and back: each continues the state it is given (t, u, v, a), bit for bit the row 0
    of its records; a resumed linear run steps on K u, not on f_int"""
    s = cases.setup("plate16", "load300")
    p, dt = s["prob"], s["dt"]
    kw = dict(dt=dt, density=RHO, probes=np.arange(2 * p.mesh.num_nodes), cg_tol=cases.CG_TOL)
    with Context(device=0) as c:
        c.upload_problem(p)
        lin = c.transient(steps=3, **kw)
        tl = c.transient(steps=3, resume=True, kinematics="tl", newton_tol=cases.NEWTON_TOL, **kw)
        back = c.transient(steps=2, resume=True, **kw)
        with pytest.raises(MagnetiteError) as e:  # (the linear run replaced the pass's own results)
            c.download_transient_tl()
        assert e.value.code == MAG_ERR_STATE
    assert tl["t_start"] == lin["t_end"] and back["t_start"] == tl["t_end"] and back["t_end"] == 8 * dt
    for k in ("u", "v", "a"):
        assert tl["probe_" + k][0].tobytes() == lin[k].tobytes() and back["probe_" + k][0].tobytes() == tl[k].tobytes(), k
    print("resumed nonlinear leg: newton", tl["newton_iterations"].tolist())
    assert tl["converged"] == 1 and tl["resumed"] == 1 and tl["iterations"][0] == 0
    lin8 = cases.linear("plate16", "load300")
    print("the state after the nonlinear leg against the linear run's", rel(tl["u"], lin8["u"][6]))
    assert rel(tl["u"], lin8["u"][6]) > 1e-6  # (the middle leg is not the linear run's: round-off would be 1e-12)


# ---- 4. the cap
def test_the_iteration_cap_is_no_error_and_leaves_the_start(built):
    s = cases.setup("beam", "beam")
    p = s["prob"]
    n2 = 2 * p.mesh.num_nodes
    with Context(device=0) as c:
        c.upload_problem(p)
        out = c.transient(steps=4, dt=s["dt"], density=RHO, probes=[1, n2 - 1], energies=True, snapshot_every=1, kinematics="tl", max_newton=2, **SET)
        start = c.transient(steps=1, dt=s["dt"], density=RHO, probes=[1, n2 - 1], energies=True, kinematics="tl", **SET)
    print("the cap:", out["message"], out["newton_residuals"])
    assert out["converged"] == 0 and out["steps"] == 0 and out["newton_iterations_total"] == 2 and out["max_step_newton"] == 2
    assert "step 1 " in out["message"] and "2 iterations" in out["message"] and "mag_run_transient_tl" in out["message"]
    assert out["newton_iterations"].tolist() == [0] and len(out["newton_residuals"]) == 2 and out["newton_residuals"][1] > cases.NEWTON_TOL
    assert out["t_end"] == 0.0 and out["probe_u"].shape == (1, 2) and out["energies"].shape == (1, 3) and out["snapshots"].shape == (1, n2)
    assert not out["u"].any() and not out["v"].any() and out["a"].any()
    for k in ("probe_u", "probe_v", "probe_a", "energies"):  # (the state is the start: row 0 of a run that goes on)
        assert out[k][0].tobytes() == start[k][0].tobytes(), k


# ---- 5. leaves the rest alone
def test_the_other_results_keep_their_bits(built):
    s = cases.setup("holes3k", "pull5")
    p = s["prob"]
    with Context(device=0) as c:
        c.upload_problem(p)
        c.run()
        before, stats = c.download(), c.stats()
        newton = c.newton(increments=1)
        c.run_modal(modes=3, density=RHO)
        modal = c.download_modal()
        for cg in (0, 4):
            out = c.transient(steps=2, dt=s["dt"], density=RHO, u0=s["u0"], kinematics="tl", cg=cg, **SET)
            assert out["converged"] == 1
            for a, b in zip(before, c.download()):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
            assert c.stats() == stats
            same_bits(c.download_newton(), {k: newton[k] for k in c.download_newton()}, "mag_download_newton")
            kept = c.download_modal()
            for k in modal:
                assert np.asarray(kept[k]).tobytes() == np.asarray(modal[k]).tobytes(), k
        c.assemble_effective_tangent(out["u"], 1.0, 1.0, RHO)
        c.run()
        for a, b in zip(before, c.download()):  # (a run afterwards is the run before)
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        again = c.download_transient_tl()
        for k in again:  # (and the pass's results survive it)
            assert np.asarray(again[k]).tobytes() == np.asarray(out[k]).tobytes(), k
        c.upload_problem(p)  # a new upload drops them
        for call in (c.download_transient_tl, c.transient_tl_info):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE


# ---- 6. device buffers
class TransientTlLeg(Leg):
    def run_transient_tl(self, steps, dt, density, amplitude=None, u0=None, v0=None, probes=None, **options):
        ins = [self._in(amplitude), self._in(u0), self._in(v0)]
        pr = None
        if probes is not None:
            pr = np.ascontiguousarray(probes, dtype=np.int32)
            pr = self.arena.put(pr, 4 if self.offset else 0) if self.device else HostBuffer(pr)
        o = _lib.TransientTlOptions()
        self.L.mag_default_transient_tl_options(C.byref(o))
        o.steps, o.dt, o.density, o.memory = int(steps), float(dt), float(density), self.memory
        o.amplitude, o.u0, o.v0, o.probes = (self._ptr(b) for b in ins + [pr])
        o.num_probes = 0 if probes is None else len(probes)
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        rc = self.L.mag_run_transient_tl(self.h, C.byref(o))
        self._called(ins + [pr], scribble=True, keep=True)
        self._transient = (o.num_probes, bool(o.energies))  # (what download_transient sizes)
        return rc

    def download_transient_tl(self, slack=3):
        info = (C.c_int32 * 8)()
        assert self.L.mag_get_transient_tl_info(self.h, info) == MAG_OK
        rows, its, E = info[0] + 1, info[3], self.ctx.E
        sizes = dict(newton_iterations=rows, cg_iterations=its, residuals=its, elem=8 * E)
        bufs = {k: self._out(n + slack, np.int32 if "iterations" in k else np.float64, (4 if self.offset else 0) if "iterations" in k else None)
                for k, n in sizes.items()}
        o = _lib.TransientTlResult()
        for k, b in bufs.items():
            setattr(o, k, self._ptr(b))
        o.memory = self.memory
        self._ok(self.L.mag_download_transient_tl(self.h, C.byref(o)))
        out = {}
        for k, flat in zip(bufs, self._called(outputs=list(bufs.values()))):
            assert (flat[sizes[k]:].view(np.uint8) == UNWRITTEN[self.memory]).all(), ("written beyond its documented size", k)
            out[k] = flat[:sizes[k]]
        out["info"] = np.array(list(info))
        return out

    def assemble_effective_tangent(self, u, c_K, c_M, density, nnz):
        ins, outs = [self._in(u)], [self._out(nnz + 3)]
        rc = self.L.mag_assemble_effective_tangent(self.h, _dp(ins[0].ptr), c_K, c_M, density, 0, _dp(outs[0].ptr), self.memory)
        val, = self._called(ins, outs, scribble=True)
        assert (val[nnz:].view(np.uint8) == UNWRITTEN[self.memory]).all(), "written beyond its documented size"
        return rc, val[:nnz]


def test_the_pass_reads_and_writes_device_memory(built):
    s = cases.setup("plate16", "pull5d")
    p = s["prob"]
    n2 = 2 * p.mesh.num_nodes
    probes = np.arange(n2 - 1, -1, -3)
    amp = np.linspace(1.0, 1.4, 6)
    v0 = 3.0 * np.cos(np.arange(n2))
    out = {}
    with DeviceArena() as arena, Context(device=0) as host, Context(device=0) as dev:
        for key, leg in (("host", TransientTlLeg(host, MAG_MEM_HOST)), ("device", TransientTlLeg(dev, MAG_MEM_DEVICE, arena, 8))):
            leg.ctx.upload_problem(p)
            nnz = len(leg.ctx.assemble_csr()[2])
            rc = leg.run_transient_tl(5, s["dt"], RHO, amp.copy(), np.array(s["u0"]), v0.copy(), probes.copy(), energies=1, snapshot_every=2,
                                      rayleigh_mass=s["alpha"], **SET)
            assert rc == MAG_OK, leg.error()
            out[key, "run"] = leg.download_transient()
            out[key, "own"] = leg.download_transient_tl()
            rc, val = leg.assemble_effective_tangent(np.array(s["u0"]), 0.25 * s["dt"] ** 2, 1.0, RHO, nnz)
            assert rc == MAG_OK, leg.error()
            out[key, "tangent"] = dict(val=val)
        arena.check()
    for part in ("run", "own", "tangent"):
        got, want = out["device", part], out["host", part]
        assert list(got) == list(want)
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (part, k)
            assert np.isfinite(got[k]).all(), (part, k)
    run, own = out["device", "run"], out["device", "own"]
    assert own["info"][0] == 5 and own["info"][7] == 1 and own["newton_iterations"][0] == 0 and own["newton_iterations"][1:].min() >= 2
    assert run["probe_u"].shape == (6, len(probes)) and np.array_equal(run["probe_u"][-1], run["u"][probes])
    assert run["snapshots"].shape == (3, n2) and np.array_equal(run["snapshots"][-1][probes], run["probe_u"][4])


# ---- 7. refusals
def test_refusals_before_any_device_work(built):
    s = cases.setup("plate16", "load300")
    p = s["prob"]
    n2 = 2 * p.mesh.num_nodes
    u = np.zeros(n2)
    ok = dict(steps=2, dt=s["dt"], density=RHO)
    with Context(device=0) as c:
        with pytest.raises(MagnetiteError, match="mag_run_transient_tl before mag_upload") as e:
            c.run_transient_tl(**ok)
        assert e.value.code == MAG_ERR_STATE
        out = np.zeros(4)
        assert c._L.mag_assemble_effective_tangent(c._h, _dp(u.ctypes.data), 1.0, 1.0, RHO, 0, _dp(out.ctypes.data), MAG_MEM_HOST) == MAG_ERR_STATE
        assert b"mag_assemble_effective_tangent before mag_upload" in c._L.mag_last_error(c._h)
        c.upload_problem(p)
        with pytest.raises(MagnetiteError, match="mag_run_transient_tl: beta = 0") as e:
            c.run_transient_tl(beta=0.0, **ok)
        assert e.value.code == MAG_ERR_BAD_ARGS and "mag_run_explicit" in e.value.message
        for kw, text in ((dict(steps=0), "steps = 0"), (dict(dt=0.0), "dt 0"), (dict(density=-1.0), "density"), (dict(beta=-0.25), "beta"),
                         (dict(gamma=float("inf")), "gamma"), (dict(rayleigh=(-1.0, 0.0)), "rayleigh_mass"), (dict(cg_tol=float("nan")), "cg_tol"),
                         (dict(newton_tol=-1.0), "newton_tol"), (dict(max_newton=-1), "max_newton = -1"), (dict(cg=5), "cg = 5 outside 0..4"),
                         (dict(snapshot_every=-1), "snapshot_every = -1")):
            with pytest.raises(MagnetiteError, match="mag_run_transient_tl") as e:
                c.run_transient_tl(**{**ok, **kw})
            assert e.value.code == MAG_ERR_BAD_ARGS and text in e.value.message, e.value.message
        with pytest.raises(MagnetiteError, match="rayleigh"):  # (the binding: the struct has no field for it)
            c.run_transient_tl(rayleigh=(0.0, 1e-7), **ok)
        o = _lib.TransientTlOptions()
        c._L.mag_default_transient_tl_options(C.byref(o))
        assert (o.steps, o.resume, o.lumped, o.cg, o.max_newton, o.beta, o.gamma, o.newton_tol, o.cg_tol, o.u0) == (0, 0, 0, 0, 0, 0.25, 0.5, 0.0, 0.0, None)
        o.steps, o.dt, o.density, o.num_probes = 2, s["dt"], RHO, 2
        assert c._L.mag_run_transient_tl(c._h, C.byref(o)) == MAG_ERR_BAD_ARGS and b"null probes" in c._L.mag_last_error(c._h)
        o.num_probes, o.memory = 0, 7
        assert c._L.mag_run_transient_tl(c._h, C.byref(o)) == MAG_ERR_BAD_ARGS and b"memory = 7" in c._L.mag_last_error(c._h)
        o.memory, o.resume = 0, 1
        assert c._L.mag_run_transient_tl(c._h, C.byref(o)) == MAG_ERR_STATE and b"resume without a completed run" in c._L.mag_last_error(c._h)
        assert c._L.mag_run_transient_tl(c._h, None) == MAG_ERR_BAD_ARGS and b"null options" in c._L.mag_last_error(c._h)
        assert c._L.mag_assemble_effective_tangent(c._h, None, 1.0, 1.0, RHO, 0, None, 0) == MAG_ERR_BAD_ARGS and b"null u" in c._L.mag_last_error(c._h)
        for call in (c.download_transient_tl, c.transient_tl_info):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE
        c.set_element_scale(np.full(p.mesh.num_elements, 0.5))
        for call in (lambda: c.run_transient_tl(**ok), lambda: c.assemble_effective_tangent(u, 1.0, 1.0, RHO)):
            with pytest.raises(MagnetiteError, match="element stiffness field") as e:
                call()
            assert e.value.code == MAG_ERR_STATE
        c.set_element_scale(None)
        c.init_callback(lambda a: None, 0, 2)
        with pytest.raises(MagnetiteError, match="communicator of 2 ranks") as e:
            c.run_transient_tl(**ok)
        assert e.value.code == MAG_ERR_BAD_ARGS
    for opts, text in ((dict(assemble_csr=0), "assemble_csr = 0"), (dict(precision=1), "precision = 1")):
        with Context(device=0, **opts) as c:
            c.upload_problem(p)
            for call in (lambda: c.run_transient_tl(**ok), lambda: c.assemble_effective_tangent(u, 1.0, 1.0, RHO)):
                with pytest.raises(MagnetiteError, match=text) as e:
                    call()
                assert e.value.code == MAG_ERR_STATE
    with Context(device=0, op_variant=1) as c:
        c.upload_problem(p)
        with pytest.raises(MagnetiteError, match="mag_run_transient_tl: cg = 2 needs the tile-local tables") as e:
            c.run_transient_tl(cg=2, **ok)
        assert e.value.code == MAG_ERR_STATE


def test_refusals_on_the_device(built):
    with Context(device=0) as c:
        c.upload_problem(meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24))))
        for call, fn in ((lambda: c.run_transient_tl(2, 1e-6, RHO), "mag_run_transient_tl"),
                         (lambda: c.assemble_effective_tangent(np.zeros(2 * c.N), 1.0, 1.0, RHO), "mag_assemble_effective_tangent")):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_BAD_ARGS and fn in e.value.message and "element 0 " in e.value.message
        p = MESHES["plate16"][0]()
        n2 = 2 * p.mesh.num_nodes
        c.upload_problem(p)
        dt = cases.setup("plate16", "pull5")["dt"]
        for probes, at in (([0, n2 - 1, n2], 2), ([-1, 3], 0)):
            with pytest.raises(MagnetiteError) as e:
                c.run_transient_tl(2, dt, RHO, probes=probes)
            assert e.value.code == MAG_ERR_BAD_ARGS and f"probes[{at}]" in e.value.message
        out = c.transient(steps=2, dt=dt, density=RHO, probes=[0, n2 - 1], kinematics="tl")
        assert out["probe_u"].shape == (3, 2) and out["converged"] == 1
        with pytest.raises(MagnetiteError):
            c.run_transient_tl(2, dt, RHO, probes=[n2])
        for call in (c.download_transient_tl, c.download_transient):  # (a refused run leaves no results of the pass)
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE
