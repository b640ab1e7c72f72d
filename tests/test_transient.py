"""No GPU: the twin of the transient pass (tests/transient_ref.py) against the closed form of the average-acceleration scheme and
its energy balance; the ABI of mag_run_transient (struct sizes against a compiled sizeof, symbols) and every error that precedes
any HIP call.

Bars.  The twin against the closed form: 1e-10 relative (measured 1.3e-12 at worst); T + W - P under a constant point load,
undamped: constant to 1e-11 of the peak strain energy (measured 6e-13 at worst)."""
import ctypes as C
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
