"""No GPU: the twin of the transient pass (tests/transient_ref.py) against the closed form of the average-acceleration scheme and
its energy balance; the ABI of mag_run_transient (struct sizes against a compiled sizeof, symbols) and every error that precedes
any HIP call.

Bars.  The twin against the closed form: 1e-10 relative (measured 1.3e-12 at worst); T + W - P under a constant point load,
undamped: constant to 1e-11 of the peak strain energy (measured 6e-13 at worst).

The stop rule's twin (transient_ref.cg_solver: field_cg_ref.fused_cg, k_cg_field's recurrence launch by launch, as the solver of
newmark()) against the LU twin, cg_tol = 1e-12, 16 steps from a moving start (transient_ref.moving_start), kinds 1 / 2 / 3, both
configs, both parameter sets.  This is what makes the GPU tests' bars (u 1e-8; v, a, reactions 1e-7) meaningful at a (mesh, dt)
pair: the bar here is a tenth of them, and a pair whose emulation misses it is no case for the GPU.  Measured, at worst over
(u | v, a, f):
    plate16  dt = T1 / 200   1.7e-13 | 5.7e-12        plate16  dt = T1 / 20   7.4e-11 | 1.5e-10
    holes3k  dt = T1 / 200   2.8e-13 | 1.5e-11        (holes3k at T1 / 20: 4.3e-10 | 2.7e-9 -- held, not used on the GPU)
At dt >= T1 the stop rule's own error (a relative residual on the right-hand side, amplified by u' = ut + beta dt^2 a') reaches
5e-5 in u: neither twin is a reference there, and no test steps that far.  Capped at 5 iterations every solve reports (5, 0)
and hands on x_5; caps 5 and 6 differ by 8e-4 .. 1.3e-2 in u and a under plain CG (1.1e-5 .. 5.6e-5 in u, 1.1e-4 .. 7.2e-4 in a
with the inverse blocks, where five iterations get closer), rounding-sized noise on the right-hand sides by 1e-13."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import modal_ref
import transient_ref as ref
from magnetite_amd import _lib, meshgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
RHO = 2700.0
UNKNOWN_MEMORY = (-1, 2, 7)  # (tests/test_memory_argument.py)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("name", ["plate16", "holes3k"])
@pytest.mark.parametrize("mode", [1, 3])
def test_the_twin_against_the_closed_form(name, mode):
    prob, K, M, free, lam, Phi = modal_ref.cached(name, RHO)
    k = mode - 1
    steps, dt = 64, 2.0 * np.pi / np.sqrt(lam[k]) / 20.0
    zero = np.zeros(K.shape[0])
    out = ref.newmark(K, M, free, zero, zero, steps, dt, u0=Phi[k])
    want = ref.mode_closed_form(lam[k], Phi[k], steps, dt)
    err = rel(out["u"], want)
    print(name, "mode", mode, "closed form", err)
    assert err <= 1e-10


@pytest.mark.parametrize("name", ["plate16", "holes3k", "frontal3k"])
def test_the_twins_energy_balance(name):
    from test_load_cases_gpu import MESHES
    prob = meshgen.config_fixed_left_point_load(MESHES[name][0]().mesh)
    K, M, free = modal_ref.matrices(prob, RHO)
    lam, _ = modal_ref.eigenpairs(K, M, free, 2)
    out = ref.newmark(K, M, free, prob.u_in, prob.f_in, 64, 2.0 * np.pi / np.sqrt(lam[0]) / 200.0)
    T, W, P = out["energies"].T
    balance = T + W - P
    drift = float(np.max(np.abs(balance - balance[0])) / W.max())
    print(name, "energy drift", drift)
    assert W.max() > 0 and drift <= 1e-11


@functools.lru_cache(maxsize=None)
def moving(name, config, lumped=False):
    """(prob, K, M, free, known, w1, T1, u0, v0) of the stop rule's tests: computed once, shared, left unchanged"""
    from test_load_cases_gpu import MESHES
    prob = MESHES[name][0]()
    if config == "load":
        prob = meshgen.config_fixed_left_point_load(prob.mesh)
    K, M, free = modal_ref.matrices(prob, RHO, lumped)
    lam, Phi = modal_ref.eigenpairs(K, M, free, 4)
    w1 = float(np.sqrt(lam[0]))
    u0, v0 = ref.moving_start(K, M, free, prob.u_in, prob.f_in, Phi, 0.05 * w1, 0.02 / w1)
    return prob, K, M, free, np.asarray(prob.u_known) != 0, w1, 2.0 * np.pi / w1, u0, v0


def parameters(which, w1):
    return (0.25, 0.5, 0.0, 0.0) if which == "undamped" else (0.3025, 0.6, 0.05 * w1, 0.02 / w1)


def amplitude_of(config, dt, T1, steps):
    return 1.0 + np.sin(2.0 * np.pi * np.arange(steps + 1) * dt / (0.7 * T1)) if config == "load" else None


@pytest.mark.parametrize("name, per_period, kinds", [("plate16", 200, (1, 2, 3)), ("plate16", 20, (1, 2, 3)), ("holes3k", 200, (1, 3))])
@pytest.mark.parametrize("config", ["load", "pull"])
@pytest.mark.parametrize("which", ["undamped", "damped"])
def test_the_stop_rules_twin_against_the_lu_twin(name, per_period, kinds, config, which):
    prob, K, M, free, known, w1, T1, u0, v0 = moving(name, config)
    steps, dt = 16, T1 / per_period
    args = (K, M, free, prob.u_in, prob.f_in, steps, dt) + parameters(which, w1) + (amplitude_of(config, dt, T1, steps),)
    assert np.isnan(u0[known]).all() and np.isnan(v0[known]).all()
    lu = ref.newmark(*args, u0=u0, v0=v0)
    # the start matters: without v0 or u0 the twin's a_0 (damped) and its reactions at step 1 are another's
    without_v0, without_u0 = ref.newmark(*args, u0=u0), ref.newmark(*args, v0=v0)
    if which == "damped":
        assert rel(without_v0["a"][0], lu["a"][0]) >= 1e-2
    assert rel(without_u0["a"][0], lu["a"][0]) >= 1e-2 and rel(without_v0["f"][1], lu["f"][1]) >= 1e-2
    for kind in kinds:
        log = []
        out = ref.newmark(*args, u0=u0, v0=v0, solver=ref.cg_solver(known, kind, 1e-12, log=log))
        worst = {k: max(rel(out[k][n], lu[k][n]) for n in range(steps + 1)) for k in ("u", "v", "a", "f")}
        print(name, config, which, "T1 /", per_period, "kind", kind, worst, "iterations", min(log)[0], "-", max(log)[0])
        assert len(log) == steps + 1 and all(c == 1 for _, c in log)
        assert worst["u"] <= 1e-9 and max(worst["v"], worst["a"], worst["f"]) <= 1e-8


@pytest.mark.parametrize("config", ["load", "pull"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_the_stop_rules_twin_at_the_cap_and_under_a_looser_tolerance(config, kind):
    prob, K, M, free, known, w1, T1, u0, v0 = moving("plate16", config)
    steps, dt = 8, T1 / 200.0
    args = (K, M, free, prob.u_in, prob.f_in, steps, dt) + parameters("damped", w1) + (amplitude_of(config, dt, T1, steps),)
    runs, logs = {}, {}
    for key, tol, cap in (("cap 5", 1e-12, 5), ("cap 6", 1e-12, 6), (1e-6, 1e-6, 10 ** 7), (1e-12, 1e-12, 10 ** 7)):
        logs[key] = []
        runs[key] = ref.newmark(*args, u0=u0, v0=v0, solver=ref.cg_solver(known, kind, tol, cap, logs[key]))
    assert logs["cap 5"] == [(5, 0)] * (steps + 1) and logs["cap 6"] == [(6, 0)] * (steps + 1)  # (no right-hand side is zero)
    for k in ("u", "a"):
        gap = rel(runs["cap 5"][k][steps], runs["cap 6"][k][steps])
        print(config, "kind", kind, k, "cap 5 against cap 6", gap)
        # plain CG: the issue's figure.  Preconditioned, five iterations get closer: what the GPU tests need is that a cap off by
        # one stands a hundred times above their bars (u 1e-8, a 1e-7)
        assert gap > (1e-4 if kind == 1 else 100 * dict(u=1e-8, a=1e-7)[k])
    loose, tight = np.array(logs[1e-6]), np.array(logs[1e-12])
    assert loose[:, 1].all() and tight[:, 1].all() and np.all(loose[:, 0] < tight[:, 0])
    assert rel(runs[1e-6]["a"][steps], runs[1e-12]["a"][steps]) > 1e-9  # (and the looser answer is another answer)


def test_struct_sizes_symbols_and_defaults(built, tmp_path):
    structs = {"mag_transient_options": _lib.TransientOptions, "mag_transient_result": _lib.TransientResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "magnetite_hip.h"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls) == 120, cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    L = _lib.lib()
    assert L.mag_version() == 4
    for name in ("mag_default_transient_options", "mag_run_transient", "mag_download_transient", "mag_get_transient_info",
                 "mag_assemble_effective"):
        assert name in _lib.SYMBOLS and getattr(L, name).argtypes is not None
    o = _lib.TransientOptions(steps=9, dt=3.0, cg=2, amplitude=1)
    L.mag_default_transient_options(C.byref(o))
    assert (o.beta, o.gamma) == (0.25, 0.5)
    for f, _ in _lib.TransientOptions._fields_:
        if f not in ("beta", "gamma"):
            assert not getattr(o, f), f
    from magnetite_amd import Context
    for method in ("run_transient", "download_transient", "transient_info", "transient", "assemble_effective"):
        assert callable(getattr(Context, method)), method


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    x = np.zeros(8)
    probes = np.zeros(4, dtype=np.int32)
    try:
        def opts(**kw):
            o = _lib.TransientOptions()
            L.mag_default_transient_options(C.byref(o))
            for k, v in {**dict(steps=4, dt=1e-5, density=RHO), **kw}.items():
                setattr(o, k, v)
            return o

        def run(o, ctx=h):
            return L.mag_run_transient(ctx, C.byref(o) if o is not None else None)

        def refused(rc, code, *words):
            msg = L.mag_last_error(h)
            assert rc == code, (rc, msg)
            for w in words:
                assert w in msg, (w, msg)

        out, info = _lib.TransientResult(), (C.c_int32 * 8)()
        dp = x.ctypes.data_as(C.POINTER(C.c_double))
        # no context
        assert run(opts(), None) == MAG_ERR_BAD_ARGS
        assert L.mag_download_transient(None, C.byref(out)) == MAG_ERR_BAD_ARGS
        assert L.mag_get_transient_info(None, info) == MAG_ERR_BAD_ARGS
        assert L.mag_assemble_effective(None, 1.0, 1.0, RHO, 0, dp, 0) == MAG_ERR_BAD_ARGS
        # a null struct
        refused(run(None), MAG_ERR_BAD_ARGS, b"mag_run_transient", b"null options")
        refused(L.mag_download_transient(h, None), MAG_ERR_BAD_ARGS, b"mag_download_transient", b"null result")
        assert L.mag_get_transient_info(h, None) == MAG_ERR_BAD_ARGS
        refused(L.mag_assemble_effective(h, 1.0, 1.0, RHO, 0, None, 0), MAG_ERR_BAD_ARGS, b"mag_assemble_effective", b"null values_out")
        # the arguments, one by one
        for steps in (0, -2):
            refused(run(opts(steps=steps)), MAG_ERR_BAD_ARGS, b"mag_run_transient", b"steps")
        for key in ("dt", "density"):
            for v in (0.0, -1.0, float("nan"), float("inf")):
                refused(run(opts(**{key: v})), MAG_ERR_BAD_ARGS, b"mag_run_transient", key.encode())
        for key in ("beta", "gamma", "rayleigh_mass", "rayleigh_stiffness", "cg_tol"):
            for v in (-1e-9, float("nan"), float("inf")):
                refused(run(opts(**{key: v})), MAG_ERR_BAD_ARGS, b"mag_run_transient", key.encode())
        for cg in (-1, 5):
            refused(run(opts(cg=cg)), MAG_ERR_BAD_ARGS, b"mag_run_transient", b"cg = ")
        refused(run(opts(snapshot_every=-1)), MAG_ERR_BAD_ARGS, b"mag_run_transient", b"snapshot_every")
        refused(run(opts(num_probes=-1)), MAG_ERR_BAD_ARGS, b"mag_run_transient", b"num_probes")
        refused(run(opts(num_probes=2)), MAG_ERR_BAD_ARGS, b"mag_run_transient", b"num_probes", b"null probes")
        for density in (0.0, -1.0, float("nan"), float("inf")):
            refused(L.mag_assemble_effective(h, 1.0, 1.0, density, 0, dp, 0), MAG_ERR_BAD_ARGS, b"mag_assemble_effective", b"density")
        refused(L.mag_assemble_effective(h, float("nan"), 1.0, RHO, 0, dp, 0), MAG_ERR_BAD_ARGS, b"mag_assemble_effective", b"c_K")
        # a memory that is none of the enum: by the header's one rule, ahead of the missing upload
        for memory in UNKNOWN_MEMORY:
            word = str(memory).encode()
            refused(run(opts(memory=memory, num_probes=2, probes=probes.ctypes.data, amplitude=x.ctypes.data)), MAG_ERR_BAD_ARGS,
                    b"mag_run_transient", b"mag_memory", word)
            refused(L.mag_download_transient(h, C.byref(_lib.TransientResult(u_out=x.ctypes.data, memory=memory))), MAG_ERR_BAD_ARGS,
                    b"mag_download_transient", b"mag_memory", word)
            refused(L.mag_assemble_effective(h, 1.0, 1.0, RHO, 0, dp, memory), MAG_ERR_BAD_ARGS, b"mag_assemble_effective", b"mag_memory", word)
        # the state: no upload, no completed run
        for memory in (_lib.MAG_MEM_HOST, _lib.MAG_MEM_DEVICE):
            refused(run(opts(memory=memory)), MAG_ERR_STATE, b"mag_run_transient before mag_upload")
            refused(L.mag_assemble_effective(h, 1.0, 1.0, RHO, 0, dp, memory), MAG_ERR_STATE, b"mag_assemble_effective before mag_upload")
            refused(L.mag_download_transient(h, C.byref(_lib.TransientResult(memory=memory))), MAG_ERR_STATE,
                    b"mag_download_transient before a completed mag_run_transient")
        refused(run(opts(resume=1)), MAG_ERR_STATE, b"mag_run_transient", b"resume without a completed run")
        refused(run(opts(resume=1, u0=x.ctypes.data)), MAG_ERR_STATE, b"mag_run_transient", b"u0 / v0 must be NULL")
        refused(run(opts(resume=1, v0=x.ctypes.data)), MAG_ERR_STATE, b"mag_run_transient", b"u0 / v0 must be NULL")
        assert L.mag_get_transient_info(h, info) == MAG_ERR_STATE
        # more than one rank
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        refused(run(opts()), MAG_ERR_BAD_ARGS, b"mag_run_transient", b"communicator")
        refused(L.mag_assemble_effective(h, 1.0, 1.0, RHO, 0, dp, 0), MAG_ERR_BAD_ARGS, b"mag_assemble_effective", b"communicator")
        refused(L.mag_download_transient(h, C.byref(out)), MAG_ERR_BAD_ARGS, b"mag_download_transient", b"communicator")
        assert L.mag_get_transient_info(h, info) == MAG_ERR_BAD_ARGS
    finally:
        L.mag_destroy(h)
    # the contexts the pass does not run on: named before the missing upload
    for kw, word in ((dict(assemble_csr=0), b"assemble_csr = 0"), (dict(precision=1), b"precision = 1")):
        o = _lib.Options()
        L.mag_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        h = L.mag_create(C.byref(o))
        assert h
        try:
            t = _lib.TransientOptions()
            L.mag_default_transient_options(C.byref(t))
            t.steps, t.dt, t.density = 4, 1e-5, RHO
            assert L.mag_run_transient(h, C.byref(t)) == MAG_ERR_STATE
            assert b"mag_run_transient" in L.mag_last_error(h) and word in L.mag_last_error(h)
            assert L.mag_assemble_effective(h, 1.0, 1.0, RHO, 0, x.ctypes.data_as(C.POINTER(C.c_double)), 0) == MAG_ERR_STATE
            assert b"mag_assemble_effective" in L.mag_last_error(h) and word in L.mag_last_error(h)
        finally:
            L.mag_destroy(h)


def test_python_mirror_asks_for_a_density_and_for_steps(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context(device=0) as c:
        c.N = 4
        with pytest.raises(MagnetiteError):
            c.run_transient(4, 1e-5)
        with pytest.raises(MagnetiteError):
            c.transient(density=RHO)
