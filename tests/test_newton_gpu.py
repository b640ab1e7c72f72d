"""GPU: mag_run_newton and mag_assemble_tangent against the numpy twin of tests/newton_ref.py: the tangent entry by entry and by a
central difference of mag_internal_force, the Newton loop on the beam, load300 and pull5 with and without tile-local tables, every
cg, the line search, the iteration cap, continuation, the same bits, no side effects, device buffers, refusals.

Bars (from the issue): the tangent 1e-12 of its largest entry (mag_internal_force's bar); the central difference 1e-8; the Newton
iteration counts equal the twin's; the twin's residual at the returned u <= 2 newton_tol ref; rel(u, u*) <= 2 newton_tol ref /
(lambda_min(K_T,FF(u*)) |u*_F|), the first-order bound, with u* the twin run on to its round-off floor; f_out on P and the element
rows against the twin at the device's own u 1e-12; the line search and the continuation reach the 8-increment equilibrium.

Measured on an MI355X (every test prints its figures before it asserts): the tangent 5.9e-16 at u = 0, 3.9e-16 at the converged
state; the central difference 7.0e-10 (plate16), 3.0e-9 (beam); Newton iteration counts equal the twin's in every case, both
contexts, every cg; the twin's residual at the returned u at most 8.2e-12 of ref; rel(u, u*) at most 1.9e-11 against bounds of
3.2e-9 to 4.7e-8; f_out on P and the element rows 2.1e-16; the beam in one increment with line_search = 10: 10 iterations, first
step 1/4, rel(u, u*) 4.5e-16; the continued run 1.9e-11."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import explicit_tl_cases as cases
import newton_ref as nr
from device_buffers import UNWRITTEN, DeviceArena, HostBuffer, Leg, _dp
from magnetite_amd import Context, MagnetiteError, _lib, meshgen
from magnetite_amd._lib import MAG_ERR_BAD_ARGS, MAG_ERR_STATE, MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK
from test_load_cases_gpu import MESHES, rel

pytestmark = pytest.mark.gpu

TOL = 1e-10
CONTEXTS = pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["tables", "op_variant1"])
SOLVES = [("beam", "beam", 8)] + [(n, "load300", 2) for n in cases.FOUR] + [(n, "pull5", 1) for n in cases.FOUR]


def device_tangent(c, u):
    rowptr, col, _ = c.assemble_csr()
    val = c.assemble_tangent(u)
    n = len(rowptr) - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n)), val


# ---- 1. the tangent, entry by entry
@pytest.mark.parametrize("name", cases.FOUR)
@CONTEXTS
def test_assemble_tangent_against_the_twin(built, name, context):
    p = nr.case_problem(name, "load300")
    a = nr.of_problem(p)
    n2 = 2 * p.mesh.num_nodes
    u = nr.case_run(name, "load300", 2)["u"]
    with Context(device=0, **context) as c:
        c.upload_problem(p)
        K_dev = c.assemble_csr()[2]
        for what, w in (("u = 0", np.zeros(n2)), ("the twin's converged u", u)):
            got, val = device_tangent(c, w)
            again = c.assemble_tangent(w)
            want = nr.tangent(*a, w)
            big = abs(want).max()
            err = abs(got - want).max() / big
            print(name, context, what, "largest entry difference / largest entry", err)
            assert err <= 1e-12
            assert val.tobytes() == again.tobytes()
            if what == "u = 0":
                err0 = np.abs(val - K_dev).max() / np.abs(K_dev).max()
                print(name, context, "K_T(0) against assemble_csr()", err0)
                assert err0 <= 1e-12
            else:
                assert np.abs(val - K_dev).max() > 1e-3 * big  # (the state matters)


# ---- 2. the tangent is the derivative of mag_internal_force
@pytest.mark.parametrize("name, kind, increments", [("plate16", "load300", 2), ("beam", "beam", 8)])
def test_the_tangent_is_the_derivative_of_the_internal_force(built, name, kind, increments):
    p = nr.case_problem(name, kind)
    u = nr.case_run(name, kind, increments)["u"]
    L = np.ptp(p.mesh.xy[:, 0])
    rng = np.random.default_rng(5)
    with Context(device=0) as c:
        c.upload_problem(p)
        KT, _ = device_tangent(c, u)
        for _ in range(3):
            d = rng.uniform(-1.0, 1.0, u.size)
            eps = 1e-6 * L
            fd = (c.internal_force(u + eps * d)[0] - c.internal_force(u - eps * d)[0]) / (2.0 * eps)
            err = np.linalg.norm(fd - KT @ d) / np.linalg.norm(KT @ d)
            print(name, "central difference of mag_internal_force against K_T d", err)
            assert err <= 1e-8


# ---- 3. the solve
def check_against_the_twin(p, out, want, floor, increments, what):
    a = nr.of_problem(p)
    known = np.asarray(p.u_known).reshape(-1) != 0
    u_star, lam_min = floor
    print(what, "newton_iterations", out["newton_iterations"], "the twin's", want["newton_iterations"], "cg", out["cg_iterations"])
    assert np.array_equal(out["newton_iterations"], want["newton_iterations"])
    rn, ref, fi = nr.residual(*a, known, p.f_in, 1.0, out["u"])
    bound = 2 * TOL * ref / (lam_min * np.linalg.norm(u_star[~known]))
    err = rel(out["u"], u_star)
    print(what, "|r_F| / ref at the returned u", rn / ref, "rel(u, u*)", err, "bound", bound)
    assert rn <= 2 * TOL * ref
    assert err <= bound
    f_err = np.linalg.norm((out["f"] - fi)[known]) / np.linalg.norm(fi[known])
    rows = nr.element_rows(*a, out["u"])
    e_err = (np.abs(out["elem"] - rows).max(axis=0) / np.abs(rows).max(axis=0)).max()
    print(what, "f_out on P", f_err, "the element rows", e_err)
    assert f_err <= 1e-12 and e_err <= 1e-12
    assert np.array_equal(out["f"][~known], np.asarray(p.f_in)[~known])
    assert np.array_equal(out["probe_u"][-1], out["u"]) and out["probe_u"].shape == (increments + 1, out["u"].size)
    assert np.array_equal(out["load"], np.arange(increments + 1) / increments)
    assert out["converged"] == 1 and out["inverted"] == 0 and out["increments_converged"] == increments and out["halvings"] == 0
    assert len(out["residuals"]) == out["newton_iterations"].sum() == out["newton_iterations_total"]
    assert (out["step_lengths"] == 1.0).all() and out["cg_iterations"].sum() == out["cg_iterations_total"]
    assert rel(out["residuals"], want["residuals"]) <= 1e-6
    assert rel(out["energies"], want["energies"]) <= 1e-9


@pytest.mark.parametrize("name, kind, increments", SOLVES)
@CONTEXTS
def test_the_solve_against_the_twin(built, name, kind, increments, context):
    p = nr.case_problem(name, kind)
    n2 = 2 * p.mesh.num_nodes
    with Context(device=0, **context) as c:
        out = c.newton(p, increments=increments, probes=np.arange(n2))
    assert (out["cg_kernel"], out["preconditioner"]) == ((3, 0) if context else (5, 2))
    check_against_the_twin(p, out, nr.case_run(name, kind, increments), nr.case_floor(name, kind, increments), increments, (name, kind, context))


@pytest.mark.parametrize("cg", [1, 2, 3, 4])
def test_every_cg_on_plate16(built, cg):
    p = nr.case_problem("plate16", "load300")
    n2 = 2 * p.mesh.num_nodes
    with Context(device=0) as c:
        out = c.newton(p, increments=2, cg=cg, probes=np.arange(n2))
    assert (out["cg_kernel"], out["preconditioner"]) == ((3, 0) if cg == 4 else (5, cg - 1))
    check_against_the_twin(p, out, nr.case_run("plate16", "load300", 2), nr.case_floor("plate16", "load300", 2), 2, ("plate16", "cg", cg))


def test_cg_1_to_3_need_the_tables(built):
    with Context(device=0, op_variant=1) as c:
        c.upload_problem(nr.case_problem("plate16", "load300"))
        with pytest.raises(MagnetiteError, match="mag_run_newton: cg = 2 needs the tile-local tables") as e:
            c.run_newton(cg=2)
        assert e.value.code == MAG_ERR_STATE


# ---- 4. line search, cap, continuation
def test_the_line_search_reaches_the_equilibrium_in_one_increment(built):
    p = nr.case_problem("beam", "beam")
    u_star, _ = nr.case_floor("beam", "beam", 8)
    with Context(device=0) as c:
        out = c.newton(p, increments=1, line_search=10)
        plain = c.newton(p, increments=8)
    err = rel(out["u"], u_star)
    print("beam, one increment, line_search = 10: iterations", out["newton_iterations"], "step lengths", out["step_lengths"], "rel(u, u*)", err)
    assert out["converged"] == 1 and out["halvings"] > 0 and out["step_lengths"].min() < 1.0 and err <= 1e-8
    assert rel(out["u"], plain["u"]) <= 1e-8


def test_the_iteration_cap_is_no_error_and_leaves_the_start(built):
    p = nr.case_problem("beam", "beam")
    n2 = 2 * p.mesh.num_nodes
    with Context(device=0) as c:
        out = c.newton(p, increments=1, max_newton=2, probes=[1, n2 - 1])
    assert out["converged"] == 0 and out["increments_converged"] == 0 and out["newton_iterations_total"] == 2
    assert not out["u"].any() and not out["probe_u"].any() and not out["load"].any() and not out["newton_iterations"].any()
    assert "increment 1 " in out["message"] and "2 iterations" in out["message"] and "mag_run_newton" in out["message"]
    assert len(out["residuals"]) == 2 and out["residuals"][1] > TOL


def test_a_run_continues_from_u0(built):
    p = nr.case_problem("beam", "beam")
    known = np.asarray(p.u_known).reshape(-1) != 0
    u_star, lam_min = nr.case_floor("beam", "beam", 8)
    ref = nr.residual(*nr.of_problem(p), known, p.f_in, 1.0, u_star)[1]
    with Context(device=0) as c:
        c.upload_problem(p)
        half = c.newton(increments=4, load_factors=np.arange(1, 5) / 8)
        rest = c.newton(increments=4, load_factors=np.arange(5, 9) / 8, u0=half["u"])
        whole = c.newton(increments=8, snapshots=True)
    err, bound = rel(rest["u"], u_star), 2 * TOL * ref / (lam_min * np.linalg.norm(u_star[~known]))
    print("continued run: rel(u, u*)", err, "bound", bound, "iterations", half["newton_iterations"], rest["newton_iterations"])
    assert half["converged"] == 1 and rest["converged"] == 1 and err <= bound
    assert np.array_equal(half["load"], np.arange(5) / 8) and np.array_equal(rest["load"][1:], np.arange(5, 9) / 8)
    assert np.array_equal(half["newton_iterations"][1:], whole["newton_iterations"][1:5])
    assert np.array_equal(rest["newton_iterations"][1:], whole["newton_iterations"][5:])
    assert half["u"].tobytes() == whole["snapshots"][4].tobytes()  # (the first half is the whole run's, bit for bit)


# ---- 5. the same bits
def same_bits(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def test_a_repeat_and_every_tile_size_give_the_same_bits(built):
    p = nr.case_problem("holes3k", "load300")
    u = nr.case_run("holes3k", "load300", 2)["u"]
    kw = dict(increments=2, probes=[0, 7], snapshots=True)
    runs, tangents = {}, {}
    for tile in (256, 512):
        with Context(device=0, tile_nodes=tile) as c:
            c.upload_problem(p)
            runs[tile] = c.newton(cg=4, **kw)
            tangents[tile] = c.assemble_tangent(u)
            if tile == 512:
                again = c.newton(cg=4, **kw)
                fused = c.newton(**kw)
                fused_again = c.newton(**kw)
    same_bits(again, runs[512], "repeat, cg = 4")
    same_bits(fused_again, fused, "repeat, cg = 0")
    same_bits(runs[256], runs[512], "tile_nodes 256 against 512, cg = 4")
    assert tangents[256].tobytes() == tangents[512].tobytes()
    assert fused["cg_kernel"] == 5 and runs[512]["cg_kernel"] == 3 and fused["snapshots"].shape == (3, u.size)
    assert np.array_equal(fused["snapshots"][-1], fused["u"]) and not fused["snapshots"][0].any()


# ---- 6. leaves the rest alone
def test_the_other_results_keep_their_bits(built):
    s = cases.setup("holes3k", "pull5")
    p = s["prob"]
    with Context(device=0) as c:
        c.upload_problem(p)
        c.run()
        before, stats = c.download(), c.stats()
        c.explicit(steps=16, density=cases.RHO, u0=s["u0"], probes=[0, 5], energies=True, snapshot_every=8, kinematics="tl")
        tr = c.download_transient()
        for cg in (0, 4):
            out = c.newton(increments=1, cg=cg)
            assert out["converged"] == 1
            kept = c.download()
            for a, b in zip(before, kept):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
            assert c.stats() == stats
            tr_after = c.download_transient()
            for k in tr:
                assert np.asarray(tr[k]).tobytes() == np.asarray(tr_after[k]).tobytes(), k
        c.assemble_tangent(out["u"])
        c.run()
        after = c.download()
        again = c.download_newton()
        for a, b in zip(before, after):  # (a run afterwards is the run before)
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        for k in again:  # (and the pass's results survive it)
            assert np.asarray(again[k]).tobytes() == np.asarray(out[k]).tobytes(), k
        c.upload_problem(p)  # a new upload drops them
        for call in (c.download_newton, c.newton_info):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE


# ---- 7. device buffers
class NewtonLeg(Leg):
    def run_newton(self, increments, load_factors=None, u0=None, probes=None, **options):
        ins = [self._in(load_factors), self._in(u0)]
        pr = None
        if probes is not None:
            pr = np.ascontiguousarray(probes, dtype=np.int32)
            pr = self.arena.put(pr, 4 if self.offset else 0) if self.device else HostBuffer(pr)
        o = _lib.NewtonOptions()
        self.L.mag_default_newton_options(C.byref(o))
        o.increments, o.memory = int(increments), self.memory
        o.load_factors, o.u0, o.probes = (self._ptr(b) for b in ins + [pr])
        o.num_probes = 0 if probes is None else len(probes)
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        rc = self.L.mag_run_newton(self.h, C.byref(o))
        self._called(ins + [pr], scribble=True)
        self._shape = (int(increments), o.num_probes, bool(o.snapshots))
        return rc

    def download_newton(self):
        increments, num_probes, snapshots = self._shape
        rows, n2, E = increments + 1, 2 * self.ctx.N, self.ctx.E
        info = (C.c_int32 * 8)()
        assert self.L.mag_get_newton_info(self.h, info) == MAG_OK
        its = info[3]
        shapes = dict(u_out=(n2 + 3,), f_out=(n2,), elem=(E, 8), probe_u=(rows, num_probes) if num_probes else None,
                      snapshots=(rows, n2) if snapshots else None, load=(rows,), energies=(rows, 2), residuals=(its,), step_lengths=(its,))
        ints = dict(newton_iterations=(rows,), cg_iterations=(its,))
        bufs = {k: self._out(v) for k, v in shapes.items()}
        bufs.update({k: self._out(v, np.int32, 4 if self.offset else 0) for k, v in ints.items()})
        o = _lib.NewtonResult()
        for k, b in bufs.items():
            setattr(o, k, self._ptr(b))
        o.memory = self.memory
        self._ok(self.L.mag_download_newton(self.h, C.byref(o)))
        keys = [k for k, b in bufs.items() if b is not None]
        out = dict(zip(keys, self._called(outputs=[bufs[k] for k in keys])))
        assert (out["u_out"][n2:].view(np.uint8) == UNWRITTEN[self.memory]).all(), "written beyond its documented size"
        out["u_out"] = out["u_out"][:n2]
        out["info"] = np.array(list(info))
        return out

    def assemble_tangent(self, u, nnz):
        ins, outs = [self._in(u)], [self._out(nnz + 3)]
        rc = self.L.mag_assemble_tangent(self.h, _dp(ins[0].ptr), _dp(outs[0].ptr), self.memory)
        val, = self._called(ins, outs, scribble=True)
        assert (val[nnz:].view(np.uint8) == UNWRITTEN[self.memory]).all(), "written beyond its documented size"
        return rc, val[:nnz]


def test_the_pass_reads_and_writes_device_memory(built):
    p = nr.case_problem("plate16", "pull5")
    n2 = 2 * p.mesh.num_nodes
    probes = np.arange(n2 - 1, -1, -3)
    factors = np.array([0.25, 0.6, 1.0])
    u0 = 0.1 * nr.case_run("plate16", "pull5", 1)["u"]
    out = {}
    with DeviceArena() as arena, Context(device=0) as host, Context(device=0) as dev:
        for key, leg in (("host", NewtonLeg(host, MAG_MEM_HOST)), ("device", NewtonLeg(dev, MAG_MEM_DEVICE, arena, 8))):
            leg.ctx.upload_problem(p)
            nnz = len(leg.ctx.assemble_csr()[2])
            assert leg.run_newton(3, factors.copy(), u0.copy(), probes.copy(), snapshots=1) == MAG_OK, leg.error()
            out[key, "run"] = leg.download_newton()
            rc, val = leg.assemble_tangent(u0.copy(), nnz)
            assert rc == MAG_OK, leg.error()
            out[key, "tangent"] = dict(val=val)
        arena.check()
    for part in ("run", "tangent"):
        got, want = out["device", part], out["host", part]
        assert list(got) == list(want)
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (part, k)
            assert np.isfinite(got[k]).all(), (part, k)
    run = out["device", "run"]
    assert run["info"][0] == 3 and run["info"][7] == 1 and np.array_equal(run["load"], np.concatenate([[0.0], factors]))
    assert run["probe_u"].shape == (4, len(probes)) and np.array_equal(run["probe_u"][-1], run["u_out"][probes])
    assert np.array_equal(run["snapshots"][0], u0) and np.array_equal(run["snapshots"][-1], run["u_out"])
    want = nr.newton(*nr.of_problem(p), p.u_known, p.u_in, p.f_in, increments=3, load_factors=factors, u0=u0)
    assert np.array_equal(run["newton_iterations"], want["newton_iterations"]) and rel(run["u_out"], want["u"]) <= 1e-8


# ---- 8. refusals
def test_refusals_before_any_device_work(built):
    p = nr.case_problem("plate16", "load300")
    n2 = 2 * p.mesh.num_nodes
    u = np.zeros(n2)
    with Context(device=0) as c:
        with pytest.raises(MagnetiteError, match="mag_run_newton before mag_upload") as e:
            c.run_newton()
        assert e.value.code == MAG_ERR_STATE
        out = np.zeros(4)
        assert c._L.mag_assemble_tangent(c._h, _dp(u.ctypes.data), _dp(out.ctypes.data), MAG_MEM_HOST) == MAG_ERR_STATE
        assert b"mag_assemble_tangent before mag_upload" in c._L.mag_last_error(c._h)
        c.upload_problem(p)
        for kw, text in ((dict(increments=0), "increments = 0"), (dict(max_newton=-1), "max_newton = -1"), (dict(line_search=-2), "line_search = -2"),
                         (dict(newton_tol=-1.0), "newton_tol"), (dict(cg_tol=float("nan")), "cg_tol"), (dict(cg=5), "cg = 5 outside 0..4")):
            with pytest.raises(MagnetiteError, match="mag_run_newton") as e:
                c.run_newton(**kw)
            assert e.value.code == MAG_ERR_BAD_ARGS and text in e.value.message, e.value.message
        o = _lib.NewtonOptions()
        c._L.mag_default_newton_options(C.byref(o))
        assert (o.increments, o.max_newton, o.line_search, o.cg, o.newton_tol, o.cg_tol, o.u0) == (1, 0, 0, 0, 0.0, 0.0, None)
        o.num_probes = 2
        assert c._L.mag_run_newton(c._h, C.byref(o)) == MAG_ERR_BAD_ARGS and b"null probes" in c._L.mag_last_error(c._h)
        o.num_probes, o.memory = 0, 7
        assert c._L.mag_run_newton(c._h, C.byref(o)) == MAG_ERR_BAD_ARGS and b"memory = 7" in c._L.mag_last_error(c._h)
        assert c._L.mag_run_newton(c._h, None) == MAG_ERR_BAD_ARGS and b"null options" in c._L.mag_last_error(c._h)
        assert c._L.mag_assemble_tangent(c._h, None, None, 0) == MAG_ERR_BAD_ARGS and b"null u" in c._L.mag_last_error(c._h)
        c.set_element_scale(np.full(p.mesh.num_elements, 0.5))
        for call in (c.run_newton, lambda: c.assemble_tangent(u)):
            with pytest.raises(MagnetiteError, match="element stiffness field") as e:
                call()
            assert e.value.code == MAG_ERR_STATE
        c.set_element_scale(None)
        c.init_callback(lambda a: None, 0, 2)
        with pytest.raises(MagnetiteError, match="communicator of 2 ranks") as e:
            c.run_newton()
        assert e.value.code == MAG_ERR_BAD_ARGS
    for opts, text in ((dict(assemble_csr=0), "assemble_csr = 0"), (dict(precision=1), "precision = 1")):
        with Context(device=0, **opts) as c:
            c.upload_problem(p)
            for call in (c.run_newton, lambda: c.assemble_tangent(u)):
                with pytest.raises(MagnetiteError, match=text) as e:
                    call()
                assert e.value.code == MAG_ERR_STATE


def test_refusals_on_the_device(built):
    with Context(device=0) as c:
        c.upload_problem(meshgen.config_fixed_left_pull_right(meshgen.clockwise(meshgen.plate(24))))
        for call, fn in ((c.run_newton, "mag_run_newton"), (lambda: c.assemble_tangent(np.zeros(2 * c.N)), "mag_assemble_tangent")):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_BAD_ARGS and fn in e.value.message and "element 0 " in e.value.message
        p = MESHES["plate16"][0]()
        n2 = 2 * p.mesh.num_nodes
        c.upload_problem(p)
        for probes, at in (([0, n2 - 1, n2], 2), ([-1, 3], 0)):
            with pytest.raises(MagnetiteError) as e:
                c.run_newton(probes=probes)
            assert e.value.code == MAG_ERR_BAD_ARGS and f"probes[{at}]" in e.value.message
        out = c.newton(probes=[0, n2 - 1])
        assert out["probe_u"].shape == (2, 2) and out["converged"] == 1
        with pytest.raises(MagnetiteError):
            c.run_newton(probes=[n2])
        with pytest.raises(MagnetiteError) as e:  # (a refused run leaves no results of the pass)
            c.download_newton()
        assert e.value.code == MAG_ERR_STATE
