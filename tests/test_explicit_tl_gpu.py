"""GPU: mag_run_explicit with kinematics = MAG_KIN_TOTAL_LAGRANGIAN and mag_internal_force against the numpy twin of
tests/explicit_tl_ref.py: the force kernel on its own, the fused kernel's force on its own, parity over the cases of
tests/explicit_tl_cases.py fused and unfused, every tile size; the same bits for a repeat, every grid and a resumed run; the
launch count; inverted elements; nothing else of the context changes; device buffers.

Bars (from the issue): mag_internal_force f 1e-12 relative L2, W 1e-13; a rigid motion |f| <= 1e-12 |K u|; the fused kernel's
a_0 1e-12; parity at every row u 1e-10, v, a, the energies and the final reactions 1e-9 (the twin's own spread under a random
renumbering is at most 1/300 of them), on the beam's 1479 steps a 1e-7 (250 times the twin's spread of 4.0e-10 there).

Measured on an MI355X (the test prints every figure before it asserts), fused | unfused.  At worst over the twelve 256-step cases:
u 5.1e-15 | 4.8e-15, v 4.5e-13 | 4.4e-13, a 3.1e-12 | 3.1e-12, the energies 2.0e-15 | 2.5e-15, the final reactions 7.8e-14 |
8.4e-14.  The beam: u 2.1e-15 | 2.2e-15, v 9.5e-12 | 9.6e-12, a 3.2e-10 | 3.5e-10, the energies 1.8e-15 | 2.0e-15, the reactions
1.2e-13 | 2.7e-13.  mag_internal_force: f 4.3e-16, W 2.2e-16, the rigid motion 2.7e-14 of |K u|; the fused kernel's a_0 4.9e-16;
tile_nodes 256 / 512 / 1024: the fused figures of their two cases; TL against linear on plate16 / pull5: 0.136 apart."""
import ctypes as C

import numpy as np
import pytest

import explicit_tl_cases as cases
from device_buffers import UNWRITTEN, DeviceArena, _dp
from magnetite_amd import Context, _lib
from magnetite_amd._lib import MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK
from test_explicit_gpu import ExplicitLeg, same_bits
from test_load_cases_gpu import rel

pytestmark = pytest.mark.gpu

RHO = cases.RHO
WORST = {}


def upload(c, prob, f_in=None):
    c.upload(prob.xy_flat, prob.conn_flat, prob.u_known, prob.u_in, prob.f_in if f_in is None else f_in, prob.youngs_modulus,
             prob.poisson_ratio, prob.part_thickness)


def final_u(name):
    """the final u of the twin's load300 run: strains of a few percent on every mesh"""
    return cases.twin(name, "load300", cases.dt_of(name, "load300"))["u"][-1]


# ---- 1. the force kernel on its own
@pytest.mark.parametrize("name", cases.FOUR)
@pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["tables", "op_variant1"])
def test_internal_force_against_the_twin(built, name, context):
    s = cases.setup(name, "load300")
    prob, K = s["prob"], s["K"]
    u = final_u(name)
    want_f, want_W, det = cases.force_of(prob, u)
    rigid = cases.rigid_motion(prob)
    with Context(device=0, **context) as c:
        upload(c, prob)
        f, W, inverted = c.internal_force(u)
        f2, W2, inverted2 = c.internal_force(u)
        fr, Wr, inverted_r = c.internal_force(rigid)
    errs = dict(f=rel(f, want_f), W=abs(W - want_W) / want_W, rigid=np.linalg.norm(fr) / np.linalg.norm(K @ rigid))
    print(name, context, "internal_force against the twin", errs, "min det F", det)
    assert errs["f"] <= 1e-12 and errs["W"] <= 1e-13 and inverted is False
    assert errs["rigid"] <= 1e-12 and inverted_r is False
    assert f.tobytes() == f2.tobytes() and W == W2 and inverted2 is False


# ---- 2. the fused kernel's force on its own
@pytest.mark.parametrize("name", cases.FOUR)
def test_the_fused_kernels_force_on_its_own(built, name):
    s = cases.setup(name, "load300")
    prob, m, free = s["prob"], s["m"], s["free"]
    n2 = 2 * prob.mesh.num_nodes
    u = final_u(name)
    want = np.zeros(n2)
    want[free] = -cases.force_of(prob, u)[0][free] / m[free]
    with Context(device=0) as c:
        upload(c, prob, np.zeros(n2))
        out = c.explicit(steps=1, density=RHO, u0=u, probes=np.arange(n2), kinematics="tl")
    err = rel(out["probe_a"][0], want)
    print(name, "a_0 of the fused kernel against -(f_int)_F / m", err)
    assert (out["method"], out["fused"]) == (7, 1) and out["inverted"] is False
    assert err <= 1e-12


# ---- 3. parity with the twin
def run_against_the_twin(name, kind, what, **context):
    s = cases.setup(name, kind)
    prob, steps = s["prob"], s["steps"]
    n2 = 2 * prob.mesh.num_nodes
    dt = cases.dt_of(name, kind)
    want = cases.twin(name, kind, dt)
    with Context(device=0, **context) as c:
        c.upload_problem(prob)
        bound = c.explicit_dt(RHO)["dt_bound"]
        out = c.explicit(steps=steps, dt=dt, density=RHO, rayleigh=(s["alpha"], 0.0), u0=s["u0"], probes=np.arange(n2), energies=True,
                         kinematics="tl")
    assert abs(dt / bound - 0.9) <= 1e-13 and out["dt"] == dt and out["dt_bound"] == bound
    worst = {}
    for k in ("u", "v", "a", "energies"):
        got = out["energies"] if k == "energies" else out["probe_" + k]
        worst[k] = max([rel(got[n], want[k][n]) for n in range(steps + 1) if np.any(want[k][n] != 0.0)], default=0.0)
    worst["f"] = rel(out["f"], want["f"][steps])
    for k in ("u", "v", "a"):
        assert np.array_equal(out[k], out["probe_" + k][steps]), k
    print(what, name, kind, "worst over the rows", worst, "min det F of the twin", want["min_det"])
    key = (what, "beam" if kind == "beam" else "256 steps")
    for k, w in worst.items():
        WORST[key + (k,)] = max(WORST.get(key + (k,), 0.0), w)
    print(what, "worst so far", {k[1:]: v for k, v in WORST.items() if k[0] == what})
    bars = dict(u=1e-10, v=1e-9, a=1e-7 if kind == "beam" else 1e-9, energies=1e-9, f=1e-9)
    for k, tol in bars.items():
        assert worst[k] <= tol, (what, name, kind, k, worst[k])
    assert out["inverted"] is False and out["finite"] == 1
    return out


@pytest.mark.parametrize("name, kind", cases.CASES)
def test_parity_with_the_twin(built, name, kind):
    out = run_against_the_twin(name, kind, "fused")
    steps = cases.setup(name, kind)["steps"]
    assert (out["method"], out["fused"], out["step_launches"], out["record_every"]) == (7, 1, steps + 1, 1)


@pytest.mark.parametrize("name, kind", cases.CASES)
def test_the_unfused_step(built, name, kind):
    out = run_against_the_twin(name, kind, "unfused", op_variant=1)
    steps = cases.setup(name, kind)["steps"]
    assert (out["method"], out["fused"], out["step_launches"]) == (7, 0, 4 * (steps + 1))


@pytest.mark.parametrize("tile", [256, 512, 1024])
@pytest.mark.parametrize("name, kind", [("holes3k", "load300"), ("two_fans", "pull5d")])
def test_every_tile_size_holds_the_bars(built, name, kind, tile):
    out = run_against_the_twin(name, kind, f"tile_nodes {tile}", tile_nodes=tile)
    assert (out["method"], out["fused"]) == (7, 1)


# ---- 4. the new ground is really new
def test_tl_and_linear_differ_and_linear_is_the_run_without_the_argument(built):
    s = cases.setup("plate16", "pull5")
    prob = s["prob"]
    n2 = 2 * prob.mesh.num_nodes
    kw = dict(steps=s["steps"], density=RHO, u0=s["u0"], probes=np.arange(0, n2, 7), energies=True, snapshot_every=64)
    with Context(device=0) as c:
        c.upload_problem(prob)
        plain = c.explicit(**kw)
        lin = c.explicit(kinematics="linear", **kw)
        tl = c.explicit(kinematics="tl", **kw)
    same_bits(lin, plain, "kinematics='linear' against no argument")
    assert (plain["method"], lin["method"], tl["method"]) == (6, 6, 7) and "inverted" not in lin and tl["inverted"] is False
    apart = rel(tl["u"], lin["u"])
    print("plate16 pull5: TL and linear final u apart by", apart)
    assert apart > 1e-2


# ---- 5. the same bits
@pytest.mark.parametrize("name", ["holes3k", "two_fans"])
def test_a_repeat_every_grid_and_a_resumed_run_give_the_same_bits(built, name, monkeypatch):
    s = cases.setup(name, "load300")
    prob = s["prob"]
    n2 = 2 * prob.mesh.num_nodes
    n1, n2_steps = 21, 27
    amp = 1.0 + 0.5 * np.sin(0.3 * np.arange(n1 + n2_steps + 1))
    kw = dict(density=RHO, rayleigh=(cases.ALPHA_PULL, 0.0), probes=np.arange(n2), energies=True, kinematics="tl")
    runs = {}
    for grid in ("1", "3", None):
        if grid is None:
            monkeypatch.delenv("MAG_TUNE_GRID", raising=False)
        else:
            monkeypatch.setenv("MAG_TUNE_GRID", grid)
        with Context(device=0) as c:
            c.upload_problem(prob)
            runs[grid] = c.explicit(steps=n1 + n2_steps, amplitude=amp, snapshot_every=3, **kw)
            if grid is None:
                again = c.explicit(steps=n1 + n2_steps, amplitude=amp, snapshot_every=3, **kw)
                first = c.explicit(steps=n1, amplitude=amp[:n1 + 1], snapshot_every=3, **kw)
                resumed_amp = amp[n1:].copy()
                resumed_amp[0] = np.nan  # (ignored: row 0 carries the load of the state it resumes)
                second = c.explicit(steps=n2_steps, amplitude=resumed_amp, snapshot_every=3, resume=True, **kw)
                c.explicit(steps=n1, amplitude=amp[:n1 + 1], **kw)
                thirds = c.explicit(steps=n2_steps, amplitude=resumed_amp, record_every=3, resume=True, **kw)
        assert runs[grid]["fused"] == 1 and runs[grid]["method"] == 7
    whole = runs[None]
    assert np.abs(whole["u"]).max() > 0
    for grid in ("1", "3"):
        same_bits(runs[grid], whole, (name, "MAG_TUNE_GRID", grid))
    same_bits(again, whole, "repeat")
    assert (first["resumed"], second["resumed"], second["step_launches"], second["method"]) == (0, 1, n2_steps, 7)
    same_bits(second, whole, "resumed", ("u", "v", "a", "f"))
    for k in ("probe_u", "probe_v", "probe_a", "energies"):
        assert first[k].tobytes() == whole[k][:n1 + 1].tobytes(), k
        assert second[k].tobytes() == whole[k][n1:].tobytes(), k
        assert thirds[k].tobytes() == whole[k][n1::3].tobytes(), k
    assert second["snapshots"].tobytes() == whole["snapshots"][n1 // 3:].tobytes()
    same_bits(thirds, whole, "resumed under another record_every", ("u", "v", "a", "f"))


def test_either_kinematics_resumes_the_others_state(built):
    s = cases.setup("plate16", "load300")
    prob = s["prob"]
    dt = cases.dt_of("plate16", "load300")
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.explicit(steps=10, dt=dt, density=RHO, kinematics="tl")
        lin = c.explicit(steps=10, dt=dt, density=RHO, resume=True)
        tl = c.explicit(steps=10, dt=dt, density=RHO, resume=True, kinematics="tl")
    assert (lin["method"], lin["resumed"], tl["method"], tl["resumed"]) == (6, 1, 7, 1)
    assert tl["t_start"] == lin["t_end"] and np.isfinite(tl["u"]).all() and np.abs(tl["u"]).max() > 0


# ---- 6. the launch count
def test_a_step_without_records_is_one_launch(built):
    prob = cases.setup("holes3k", "load300")["prob"]
    with Context(device=0) as c:
        c.upload_problem(prob)
        out = c.explicit(steps=37, density=RHO, kinematics="tl")
        info = (C.c_int32 * 8)()
        assert c._L.mag_get_transient_info(c._h, info) == MAG_OK
    assert (info[1], info[2], info[3]) == (7, 1, 38)
    assert (out["method"], out["fused"], out["step_launches"], out["finite"], out["inverted"]) == (7, 1, 38, 1, False)


# ---- 7. inverted elements
@pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["fused", "unfused"])
def test_an_inverted_element_is_flagged_and_is_no_error(built, context):
    prob = cases.setup("plate16", "load300")["prob"]
    n2 = 2 * prob.mesh.num_nodes
    u0 = np.zeros(n2)
    u0[2 * (8 * 17 + 8)] = 1.5 / 16  # (an interior node, 1.5 cell widths in x)
    with Context(device=0, **context) as c:
        c.upload_problem(prob)
        bound = c.explicit_dt(RHO)["dt_bound"]
        out = c.explicit(steps=1, dt=1e-3 * bound, density=RHO, u0=u0, kinematics="tl")
        info = (C.c_int32 * 8)()
        assert c._L.mag_get_transient_info(c._h, info) == MAG_OK
        f, W, inverted = c.internal_force(u0)
    assert info[7] == 0 and out["inverted"] is True and inverted is True
    for k in ("u", "v", "a", "f"):
        assert np.isfinite(out[k]).all(), k
    assert np.isfinite(f).all() and np.isfinite(W)


# ---- 8. leaves the rest alone
def test_the_other_results_keep_their_bits(built):
    s = cases.setup("holes3k", "pull5")
    prob = s["prob"]
    with Context(device=0) as c:
        c.upload_problem(prob)
        c.run()
        before = c.download()
        out = c.explicit(steps=32, density=RHO, u0=s["u0"], probes=[0, 5], energies=True, snapshot_every=8, kinematics="tl")
        tr = c.download_transient()
        c.internal_force(s["u0"])
        c.run()
        after = c.download()
        tr_after = c.download_transient()
    assert np.abs(out["v"]).max() > 0
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    for k in tr:  # (mag_internal_force changes no result of the pass either)
        assert np.asarray(tr[k]).tobytes() == np.asarray(tr_after[k]).tobytes(), k


# ---- 9. device buffers
class TlLeg(ExplicitLeg):
    def internal_force(self, u):
        ins = [self._in(u)]
        outs = [self._out(2 * self.ctx.N + 3)]
        scalars = np.full(2, np.nan)
        rc = self.L.mag_internal_force(self.h, _dp(ins[0].ptr), _dp(outs[0].ptr), scalars.ctypes.data_as(C.POINTER(C.c_double)), self.memory)
        f, = self._called(ins, outs, scribble=True)
        n2 = 2 * self.ctx.N
        assert (f[n2:].view(np.uint8) == UNWRITTEN[self.memory]).all(), "written beyond its documented size"
        return rc, f[:n2], scalars


def test_the_pass_reads_and_writes_device_memory(built):
    s = cases.setup("plate16", "pull5d")
    prob = s["prob"]
    n2 = 2 * prob.mesh.num_nodes
    probes = np.arange(n2 - 1, -1, -3)
    u0 = s["u0"].copy()  # (the legs scribble over their inputs: never the shared array)
    opts = dict(rayleigh_mass=s["alpha"], energies=1, snapshot_every=3, kinematics=_lib.MAG_KIN_TOTAL_LAGRANGIAN)
    amp = 1.0 + 0.25 * np.cos(0.4 * np.arange(16))
    resumed_amp = amp[10:].copy()
    resumed_amp[0] = np.nan
    out = {}
    with DeviceArena() as arena, Context(device=0) as host, Context(device=0) as dev:
        for key, leg in (("host", TlLeg(host, MAG_MEM_HOST)), ("device", TlLeg(dev, MAG_MEM_DEVICE, arena, 8))):
            leg.ctx.upload_problem(prob)
            assert leg.run_explicit(10, RHO, amp[:11].copy(), u0.copy(), None, probes.copy(), **opts) == MAG_OK, leg.error()
            out[key, "first"] = leg.download_transient()
            assert leg.run_explicit(5, RHO, resumed_amp.copy(), probes=probes[:7].copy(), resume=1, **opts) == MAG_OK, leg.error()
            out[key, "resumed"] = leg.download_transient()
            rc, f, scalars = leg.internal_force(u0.copy())
            assert rc == MAG_OK, leg.error()
            out[key, "force"] = dict(f=f, scalars=scalars)
        arena.check()
    for part in ("first", "resumed", "force"):
        got, want = out["device", part], out["host", part]
        assert list(got) == list(want)
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (part, k)
            if isinstance(got[k], np.ndarray) and got[k].dtype == np.float64:
                assert np.isfinite(got[k]).all(), (part, k)
    assert out["device", "first"]["probe_u"].shape == (11, len(probes)) and out["device", "first"]["snapshots"].shape == (4, n2)
    assert out["device", "resumed"]["probe_u"].shape == (6, 7) and np.any(out["device", "resumed"]["v"] != 0.0)
    want_f, want_W, det = cases.force_of(prob, u0)
    assert rel(out["device", "force"]["f"], want_f) <= 1e-12 and out["device", "force"]["scalars"][1] == 0.0
    assert abs(out["device", "force"]["scalars"][0] - want_W) <= 1e-13 * want_W
