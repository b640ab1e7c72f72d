"""No GPU: the twin of the explicit pass (tests/explicit_ref.py) against the Newmark twin at beta = 0 on the lumped mass, the
bound of the stable step against the true limit, stability on either side of the limit, the closed form of a lumped-mass mode;
the ABI of mag_run_explicit (struct layout against a compiled offsetof, symbols, defaults), every error that precedes any HIP
call and the Python mirror's argument checks (the tool's --dry-run parse: tests/test_explicit_cpp.py).

Bars (from the issue) and what was measured:
  the twin against transient_ref.newmark(beta=0, gamma=0.5) at eta = 0, 64 steps at 0.9 dt_bound: 1e-13 in u, v, a and the
    energies (worst 6.4e-15 / 2.3e-14 / 6.3e-14 / 9.5e-16; the reactions, a cancelling sum, to the bar times their amplification);
  dt_bound / (2 / omega_max) in [0.6, 1] on the four meshes, both configs (0.69 .. 0.94);
  3000 steps at 0.98 of the damped limit formed with the true omega_max stay bounded, at 1.03 they grow (undamped: 0.999, 1.02);
  the closed form over 64 steps: 1e-11 of max|phi| (worst 1.0e-13)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import explicit_cases as cases
import explicit_ref as ref
import modal_ref
import transient_ref
from magnetite_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7
RHO = cases.RHO
UNKNOWN_MEMORY = (-1, 2, 7)  # (tests/test_memory_argument.py)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("name, config", cases.CASES)
@pytest.mark.parametrize("which", ["undamped", "mass-damped"])
def test_the_twin_is_newmark_with_beta_zero_on_the_lumped_mass(name, config, which):
    prob, K, M, m, free, w1, T1 = cases.setup(name, config)
    alpha = 0.0 if which == "undamped" else 0.05 * w1
    steps, dt = 64, 0.9 * ref.bound(K, m, free)
    amp = cases.amplitude_of(config, dt, T1, steps)
    got = ref.explicit(K, M, free, prob.u_in, prob.f_in, steps, dt, alpha, 0.0, amp)
    want = transient_ref.newmark(K, M, free, prob.u_in, prob.f_in, steps, dt, 0.0, 0.5, alpha, 0.0, amp)
    worst = {k: max(rel(got[k][n], want[k][n]) for n in range(steps + 1) if np.any(want[k][n] != 0.0)) for k in ("u", "v", "a")}
    worst["energies"] = rel(got["energies"], want["energies"])
    # The reactions are no part of the scheme: on P they are K u, a sum that cancels.  A difference of u is amplified by
    # kappa = | |K| |u| |_P / |K u|_P (119 on holes3k as uploaded, where u differs by 8e-16 and f by 2.4e-13): f is held to the
    # bar times kappa, row by row
    known = np.ones(K.shape[0], dtype=bool)
    known[free] = False
    worst["f / kappa"] = 0.0
    for n in range(steps + 1):
        if np.any(want["f"][n] != 0.0):
            kappa = max(1.0, np.linalg.norm((abs(K) @ np.abs(want["u"][n]))[known]) / max(np.linalg.norm((K @ want["u"][n])[known]), 1e-300))
            worst["f / kappa"] = max(worst["f / kappa"], rel(got["f"][n], want["f"][n]) / kappa)
    print(name, config, which, worst)
    assert max(worst.values()) <= 1e-13


@pytest.mark.parametrize("name, config", [c for c in cases.CASES if c[0] != "rollers"])
def test_the_bound_is_below_the_true_limit_and_not_far_below(name, config):
    prob, K, M, m, free, w1, T1 = cases.setup(name, config)
    share = ref.bound(K, m, free) / (2.0 / cases.omega_max(name, config))
    print(name, config, "dt_bound / (2 / omega_max)", share, "T1 / dt_bound", T1 / ref.bound(K, m, free))
    assert 0.6 <= share <= 1.0
    # the lagged stiffness part shrinks the limit, the bound with it; never above the damped limit either
    eta = 0.02 / w1
    assert ref.bound(K, m, free, eta) < ref.bound(K, m, free)
    assert ref.bound(K, m, free, eta) <= ref.dt_limit(cases.omega_max(name, config), eta)


@pytest.mark.parametrize("name", ["plate16", "rollers"])
@pytest.mark.parametrize("which, below, above", [("damped", 0.98, 1.03), ("undamped", 0.999, 1.02)])
def test_the_twin_is_stable_below_the_true_limit_and_grows_above(name, which, below, above):
    prob, K, M, m, free, w1, T1 = cases.setup(name, "load")
    alpha, eta = cases.rayleigh(which, w1)
    limit = ref.dt_limit(cases.omega_max(name, "load"), eta)
    steps = 3000
    size = {}
    for share in (below, above):
        with np.errstate(all="ignore"):  # (above the limit the twin overflows: that is the point)
            out = ref.explicit(K, M, free, prob.u_in, prob.f_in, steps, share * limit, alpha, eta)
        size[share] = np.abs(out["u"]).max(axis=1)
    static = size[below][: steps // 3].max()  # (the response of the first thousand steps)
    print(name, which, "largest |u|: first third", static, "below", size[below].max(), "above", size[above][-1])
    assert np.isfinite(size[below]).all() and size[below].max() <= 4.0 * static
    assert not np.isfinite(size[above][-1]) or size[above][-1] >= 1e6 * static


@pytest.mark.parametrize("name", ["plate16", "holes3k"])
@pytest.mark.parametrize("mode", [1, 2])
def test_the_twin_against_the_closed_form(name, mode):
    prob, K, M, free, lam, Phi = modal_ref.cached(name, RHO, True)
    k = mode - 1
    steps, dt = 64, 0.9 * ref.bound(K, M.diagonal(), free)
    zero = np.zeros(K.shape[0])
    out = ref.explicit(K, M, free, zero, zero, steps, dt, u0=Phi[k])
    want = ref.mode_closed_form(lam[k], Phi[k], steps, dt)
    err = float(np.abs(out["u"] - want).max() / np.abs(Phi[k]).max())
    print(name, "mode", mode, "closed form", err)
    assert err <= 1e-11


def test_struct_layout_symbols_and_defaults(built, tmp_path):
    cname, cls = "mag_explicit_options", _lib.ExplicitOptions
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "magnetite_hip.h"', "int main(void){",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for f, _ in cls._fields_:
        lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 104
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    L = _lib.lib()
    assert L.mag_version() == 4
    for name in ("mag_default_explicit_options", "mag_run_explicit", "mag_explicit_dt"):
        assert name in _lib.SYMBOLS and getattr(L, name).argtypes is not None
    o = _lib.ExplicitOptions(steps=9, dt=3.0, energies=2, amplitude=1)
    L.mag_default_explicit_options(C.byref(o))
    assert (o.record_every, o.dt_scale) == (1, 0.9)
    for f, _ in cls._fields_:
        if f not in ("record_every", "dt_scale"):
            assert not getattr(o, f), f
    from magnetite_amd import Context
    for method in ("run_explicit", "explicit", "explicit_dt"):
        assert callable(getattr(Context, method)), method
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    assert "explicit stepping without a solve" not in header


def test_errors_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    x = np.zeros(8)
    probes = np.zeros(4, dtype=np.int32)
    out4 = (C.c_double * 4)()
    try:
        def opts(**kw):
            o = _lib.ExplicitOptions()
            L.mag_default_explicit_options(C.byref(o))
            for k, v in {**dict(steps=4, density=RHO), **kw}.items():
                setattr(o, k, v)
            return o

        def run(o, ctx=h):
            return L.mag_run_explicit(ctx, C.byref(o) if o is not None else None)

        def refused(rc, code, *words):
            msg = L.mag_last_error(h)
            assert rc == code, (rc, msg)
            for w in words:
                assert w in msg, (w, msg)

        # no context
        assert run(opts(), None) == MAG_ERR_BAD_ARGS
        assert L.mag_explicit_dt(None, RHO, 0.0, out4) == MAG_ERR_BAD_ARGS
        # a null struct
        refused(run(None), MAG_ERR_BAD_ARGS, b"mag_run_explicit", b"null options")
        refused(L.mag_explicit_dt(h, RHO, 0.0, None), MAG_ERR_BAD_ARGS, b"mag_explicit_dt", b"null out")
        # the arguments, one by one
        for steps in (0, -2):
            refused(run(opts(steps=steps)), MAG_ERR_BAD_ARGS, b"mag_run_explicit", b"steps")
        for key in ("dt", "dt_scale", "rayleigh_mass", "rayleigh_stiffness"):
            for v in (-1e-9, float("nan"), float("inf")):
                refused(run(opts(**{key: v})), MAG_ERR_BAD_ARGS, b"mag_run_explicit", key.encode())
        for v in (0.0, -1.0, float("nan"), float("inf")):
            refused(run(opts(density=v)), MAG_ERR_BAD_ARGS, b"mag_run_explicit", b"density")
            refused(L.mag_explicit_dt(h, v, 0.0, out4), MAG_ERR_BAD_ARGS, b"mag_explicit_dt", b"density")
        for v in (-1e-9, float("nan"), float("inf")):
            refused(L.mag_explicit_dt(h, RHO, v, out4), MAG_ERR_BAD_ARGS, b"mag_explicit_dt", b"rayleigh_stiffness")
        for key in ("record_every", "snapshot_every", "num_probes"):
            refused(run(opts(**{key: -1})), MAG_ERR_BAD_ARGS, b"mag_run_explicit", key.encode())
        refused(run(opts(num_probes=2)), MAG_ERR_BAD_ARGS, b"mag_run_explicit", b"num_probes", b"null probes")
        # a memory that is none of the enum: by the header's one rule, ahead of the missing upload
        for memory in UNKNOWN_MEMORY:
            refused(run(opts(memory=memory, num_probes=2, probes=probes.ctypes.data, amplitude=x.ctypes.data)), MAG_ERR_BAD_ARGS,
                    b"mag_run_explicit", b"mag_memory", str(memory).encode())
        # the state: no upload, no completed run
        for memory in (_lib.MAG_MEM_HOST, _lib.MAG_MEM_DEVICE):
            refused(run(opts(memory=memory)), MAG_ERR_STATE, b"mag_run_explicit before mag_upload")
        refused(L.mag_explicit_dt(h, RHO, 0.0, out4), MAG_ERR_STATE, b"mag_explicit_dt before mag_upload")
        refused(run(opts(resume=1)), MAG_ERR_STATE, b"mag_run_explicit", b"resume without a completed run")
        refused(run(opts(resume=1, u0=x.ctypes.data)), MAG_ERR_STATE, b"mag_run_explicit", b"u0 / v0 must be NULL")
        refused(run(opts(resume=1, v0=x.ctypes.data)), MAG_ERR_STATE, b"mag_run_explicit", b"u0 / v0 must be NULL")
        # more than one rank
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count: 0)
        assert L.mag_comm_init_callback(h, 2, 0, cb, None) == 0
        refused(run(opts()), MAG_ERR_BAD_ARGS, b"mag_run_explicit", b"communicator")
        refused(L.mag_explicit_dt(h, RHO, 0.0, out4), MAG_ERR_BAD_ARGS, b"mag_explicit_dt", b"communicator")
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
            t = _lib.ExplicitOptions()
            L.mag_default_explicit_options(C.byref(t))
            t.steps, t.density = 4, RHO
            assert L.mag_run_explicit(h, C.byref(t)) == MAG_ERR_STATE
            assert b"mag_run_explicit" in L.mag_last_error(h) and word in L.mag_last_error(h)
            assert L.mag_explicit_dt(h, RHO, 0.0, out4) == MAG_ERR_STATE
            assert b"mag_explicit_dt" in L.mag_last_error(h) and word in L.mag_last_error(h)
        finally:
            L.mag_destroy(h)


def test_python_mirror_asks_for_a_density_steps_and_whole_arrays(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context(device=0) as c:
        c.N = 4
        with pytest.raises(MagnetiteError, match="density"):
            c.run_explicit(4)
        with pytest.raises(MagnetiteError, match="steps"):
            c.explicit(density=RHO)
        with pytest.raises(MagnetiteError, match="5 entries where 8"):
            c.run_explicit(4, density=RHO, u0=np.zeros(5))
        with pytest.raises(MagnetiteError, match="4 entries where 5"):
            c.run_explicit(4, density=RHO, amplitude=np.ones(4))
