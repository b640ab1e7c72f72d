"""GPU: the neo-Hooke material of the total-Lagrangian passes (mag_set_material_law) against the numpy twin of tests/hyper_ref.py --
force, energy, tangent and element rows entry by entry, the tangent as the derivative of the force, mag_run_newton, mag_run_explicit
and mag_run_transient_tl on the issue's cases, and the law as context state: the default, the bits under St. Venant-Kirchhoff, the
other passes' results, uploads, refusals, device buffers.

Bars.  Force, W, tangent, element rows, and the explicit run (which only evaluates forces): the device is measured against the
twin's formulas evaluated in np.longdouble, and the bar is 4 times the float64 twin's own distance from that evaluation on the same
case, over the largest entry (SPREAD, EXPLICIT_SPREAD: measured on the CPU, the constants below; 4x covers the device's other
summation order and nothing more; the scalar W is held to 4 max(its spread, eps / 2): the twin's 0.3 ulp on holes3k and frontal3k
is chance, the device's 1.3 ulp is a double's rounding).  The solves: the twin is run on until its residual stops falling; FLOOR is the level it stays at
(|r_F| / ref).  The device run with newton_tol = 4 FLOOR must converge -- it reaches the twin's floor within the factor --, and its
state is then within the first-order bound 4 FLOOR ref / (lambda_min |x_F|) of the twin's floor state, lambda_min the smallest
eigenvalue of the matrix of the last iteration; the transient run carries a step's error on: n steps give n times the bound for
a, n c_v times it for v and 3 n^2 c_u times it for u (dt c_v = 2 c_u under gamma = 1/2, beta = 1/4).  At the default tolerances
the device takes the twin's iteration counts.  The central difference: h = 1e-6 L leaves eps |f| / (h |K d|), 2e-10, times the lever
of an element (L / edge, at most 32): 1e-8, mag_run_newton's bar.  Every figure is printed before it is asserted.

Measured on an MI355X, at worst over the cases and both contexts: force 8.9e-16, W 3.1e-16, tangent 5.0e-16, element rows 1.5e-15;
the central difference 3.9e-9; Newton iteration counts the twin's in every increment and step; run on to the floor, rel(u, u*) 5e-17
to 1.9e-15 against bounds of 1.7e-14 to 4.3e-11, the transient run u 4.9e-13, v 2.9e-12, a 2.0e-12 against 6.5e-11 and more; the
explicit run u 8.9e-16, v 2.3e-13, a 5.9e-12, reactions 4.8e-14, energies 6.5e-16; the effective tangent no entry of other bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import explicit_tl_cases as tlc
import hyper_ref as hr
import newton_ref as nr
import transient_tl_cases as ttc
from device_buffers import DeviceArena, _dp
from magnetite_amd import Context, MagnetiteError, meshgen
from magnetite_amd._lib import MAG_ERR_BAD_ARGS, MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK

pytestmark = pytest.mark.gpu

NH = "neo_hooke"
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
RHO = tlc.RHO
CONTEXTS = pytest.mark.parametrize("context", [{}, dict(op_variant=1)], ids=["tables", "op_variant1"])
MESHES = list(tlc.FOUR) + ["beam", "strip"]

# the float64 twin's distance from its formulas in np.longdouble at hr.finite_state(p, 0.1), over the largest entry (hr.spread):
#            force     W         tangent   element rows (hr.rows_distance)
SPREAD = {
    "plate16":   (1.50e-15, 1.33e-16, 4.91e-16, 1.76e-15),
    "holes3k":   (2.03e-15, 6.46e-17, 6.32e-16, 2.07e-15),
    "frontal3k": (2.48e-15, 5.57e-17, 3.08e-16, 1.78e-15),
    "two_fans":  (2.07e-15, 1.27e-16, 4.91e-16, 1.85e-15),
    "beam":      (1.52e-15, 1.38e-16, 4.56e-16, 2.35e-15),
    "strip":     (9.91e-16, 8.36e-17, 4.69e-16, 1.56e-15),
}
# the level the twin's |r_F| / ref stays at when mag_run_newton's cases are run on past convergence (4 more iterations)
FLOOR = {("beam", "beam", 8): 1.68e-13, ("strip", "strip", 4): 8.27e-16, ("plate16", "load300", 2): 9.16e-15,
         ("holes3k", "load300", 2): 1.14e-14, ("frontal3k", "load300", 2): 1.11e-14, ("two_fans", "load300", 2): 1.03e-14}
# the float64 explicit twin against the same loop in np.longdouble, the worst row: u, v, a, the final reactions on P, the energies
EXPLICIT_SPREAD = {
    ("plate16", "pull5"):   (1.05e-15, 8.05e-14, 3.92e-13, 8.00e-15, 9.13e-16),
    ("frontal3k", "pull5"): (7.84e-16, 2.35e-13, 1.41e-12, 5.16e-14, 3.28e-16),
    ("beam", "beam"):       (1.79e-14, 6.68e-14, 8.47e-12, 2.48e-14, 8.10e-16),
}
EXPLICIT_STEPS = 256
TRANSIENT_STEPS = 8
# the twin's |r| / ref at its floor over the 8 steps of the beam at T1 / 20 (consistent, lumped)
TRANSIENT_FLOOR = {False: 7.7e-12, True: 8.9e-12}  # (c_u K_T dominates A_T at this step: eps |A_T| |a| is far above eps ref)


def kind_of(name):
    return "beam" if name == "beam" else ("strip" if name == "strip" else "load300")


def rel(a, b):
    n = float(np.linalg.norm(np.asarray(b, dtype=LD)))
    d = float(np.linalg.norm(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)))
    return d / n if n > 0 else d


def neo_context(**opts):
    c = Context(device=0, **opts)
    c.set_material_law(NH)
    return c


def device_csr(c, val):
    rowptr, col, _ = c.assemble_csr()
    n = len(rowptr) - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n))


@functools.lru_cache(maxsize=None)
def exact(name):
    """the twin in np.longdouble at the mesh's finite state: (u, f, W, K as float64 CSR of the longdouble values, rows, min det F)"""
    p = hr.case_problem(name, kind_of(name))
    a = hr.of_problem(p)
    u = hr.finite_state(p, 0.1)
    f, W, det = hr.neo_force(*a, u, LD)
    rowptr, col, val = hr.neo_tangent(*a, u, LD)
    n = 2 * p.mesh.num_nodes
    return u, f, W, sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(n, n)), hr.neo_element_rows(*a, u, LD), det


# ---- 1. force, energy, tangent, entry by entry
@pytest.mark.parametrize("name", MESHES)
@CONTEXTS
def test_force_energy_and_tangent_against_the_twin(built, name, context):
    p = hr.case_problem(name, kind_of(name))
    u, f, W, K, _, det = exact(name)
    s_f, s_W, s_K, _ = SPREAD[name]
    with neo_context(**context) as c:
        c.upload_problem(p)
        got_f, got_W, inverted = c.internal_force(u)
        val = c.assemble_tangent(u)
        got_K = device_csr(c, val)
        zero_f, zero_W, _ = c.internal_force(np.zeros_like(u))
        K0, K_lin = c.assemble_tangent(np.zeros_like(u)), c.assemble_csr()[2]
        again = c.assemble_tangent(u)
    err_f = float(np.abs(got_f - f).max() / np.abs(f).max())
    err_W = float(abs(got_W - W) / abs(W))
    err_K = float(abs(got_K - K).max() / abs(K).max())
    err_0 = float(np.abs(K0 - K_lin).max() / np.abs(K_lin).max())
    # (W is one float64: its distance from the exact value is not measurable below half an ulp, whatever the twin's happened to be)
    bar_W = 4 * max(s_W, EPS / 2)
    # an entry of K_T sums at most `valence` triangles, each a few (8) roundings of terms of the largest entry's size
    valence = int(np.bincount(np.asarray(p.mesh.conn).reshape(-1)).max())
    err_T = float(abs(got_K - got_K.T).max() / abs(K).max())
    print(name, context, "force", err_f, "bar", 4 * s_f, "W", err_W, "bar", bar_W, "tangent", err_K, "bar", 4 * s_K, "K_T(0) against K", err_0,
          "asymmetry", err_T, "bar", 8 * valence * EPS, "min det F", det)
    assert err_f <= 4 * s_f and err_W <= bar_W and err_K <= 4 * s_K
    assert not inverted and det > 0
    assert not zero_f.any() and zero_W == 0.0  # (u = 0 gives exactly zero)
    assert err_0 <= 1e-12 and err_T <= 8 * valence * EPS  # (K_T(0) = K: mag_assemble_tangent's bar for the same identity)
    assert val.tobytes() == again.tobytes()


def test_an_inverted_element_raises_the_flag_and_gives_finite_numbers(built):
    p = hr.case_problem("plate16", "load300")
    a = hr.of_problem(p)
    u = hr.finite_state(p, 0.05).reshape(-1, 2)
    tri = p.mesh.conn[7]
    u[tri[0]] += 1.6 * (0.5 * (p.mesh.xy[tri[1]] + p.mesh.xy[tri[2]]) - p.mesh.xy[tri[0]])  # (a corner through the opposite edge)
    u = u.reshape(-1)
    f, W, det = hr.neo_force(*a, u, LD)
    with neo_context() as c:
        c.upload_problem(p)
        got_f, got_W, inverted = c.internal_force(u)
        val = c.assemble_tangent(u)
    err = float(np.abs(got_f - f).max() / np.abs(f).max())
    print("inverted element: min det F", det, "force against the twin", err, "W", float(abs(got_W - W) / abs(W)))
    assert det < 0 and inverted and np.isfinite(got_f).all() and np.isfinite(val).all() and np.isfinite(got_W)
    assert err <= 1e-12  # (j2 = (det F)^2: the same formulas; the state is no case of SPREAD, so mag_internal_force's bar)


# ---- 2. the effective tangent has the bits of the two-kernel path
@pytest.mark.parametrize("name", ["plate16", "holes3k"])
@CONTEXTS
def test_the_effective_tangent_bit_for_bit(built, name, context):
    p = hr.case_problem(name, "load300")
    u = exact(name)[0]
    with neo_context(**context) as c:
        c.upload_problem(p)
        rowptr, col, _ = c.assemble_csr()
        row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
        on = (row & 1) == (np.asarray(col) & 1)
        for lumped, (c_K, c_M) in ((False, (2.5e-11, 1.0)), (True, (3e-11, 1.01))):
            got = c.assemble_effective_tangent(u, c_K, c_M, RHO, lumped)
            ck = c_K * c.assemble_tangent(u)
            want = np.where(on, ck + c_M * c.assemble_effective(0.0, 1.0, RHO, lumped), ck)
            differ = int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
            print(name, context, "lumped" if lumped else "consistent", "entries of other bits", differ, "of", got.size)
            assert differ == 0
        c.set_material_law("svk")
        assert np.abs(c.assemble_effective_tangent(u, 1.0, 0.0, RHO) - ck / c_K).max() > 0  # (the law matters)


# ---- 3. the device tangent is the central difference of the device force
@pytest.mark.parametrize("name", ["plate16", "beam", "strip"])
def test_the_tangent_is_the_derivative_of_the_force(built, name):
    p = hr.case_problem(name, kind_of(name))
    u = exact(name)[0]
    L = np.ptp(p.mesh.xy[:, 0])
    rng = np.random.default_rng(5)
    with neo_context() as c:
        c.upload_problem(p)
        KT = device_csr(c, c.assemble_tangent(u))
        for _ in range(3):
            d = rng.uniform(-1.0, 1.0, u.size)
            eps = 1e-6 * L
            fd = (c.internal_force(u + eps * d)[0] - c.internal_force(u - eps * d)[0]) / (2.0 * eps)
            err = np.linalg.norm(fd - KT @ d) / np.linalg.norm(KT @ d)
            print(name, "central difference of mag_internal_force against K_T d", err)
            assert err <= 1e-8


# ---- 4. mag_run_newton
NEWTON_CASES = [("beam", "beam", 8), ("strip", "strip", 4)] + [(n, "load300", 2) for n in tlc.FOUR]


@functools.lru_cache(maxsize=None)
def newton_floor(name, kind, increments):
    """the twin run on (4 iterations past convergence in the last increment): u*, lambda_min(K_T,FF(u*)), ref"""
    p = hr.case_problem(name, kind)
    a = hr.of_problem(p)
    out = hr.case_run(NH, name, kind, increments, 0, 4)
    known = np.asarray(p.u_known).reshape(-1) != 0
    free = np.flatnonzero(~known)
    K = hr.tangent(NH, *a, out["u"])[free][:, free].tocsc()
    lam_min = float(spla.eigsh(K, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    fi = hr.force(NH, *a, out["u"])[0]
    ref = max(np.linalg.norm(np.where(known, 0.0, p.f_in)), np.linalg.norm(np.where(known, fi, 0.0)))
    return out["u"], lam_min, float(ref), out


@pytest.mark.parametrize("name, kind, increments", NEWTON_CASES)
@CONTEXTS
def test_newton_against_the_twin(built, name, kind, increments, context):
    p = hr.case_problem(name, kind)
    a = hr.of_problem(p)
    n2 = 2 * p.mesh.num_nodes
    known = np.asarray(p.u_known).reshape(-1) != 0
    want = hr.case_run(NH, name, kind, increments)
    u_star, lam_min, ref, floor_run = newton_floor(name, kind, increments)
    bar_r = 4 * FLOOR[(name, kind, increments)]
    with neo_context(**context) as c:
        out = c.newton(p, increments=increments, probes=np.arange(n2))
        on = c.newton(increments=increments, newton_tol=bar_r, cg_tol=1e-12)
    print(name, kind, context, "newton_iterations", out["newton_iterations"], "the twin's", want["newton_iterations"], "run on", on["newton_iterations"])
    assert out["material"] == NH and out["converged"] == 1 and out["halvings"] == 0
    assert np.array_equal(out["newton_iterations"], want["newton_iterations"])
    assert (out["inverted"] != 0) == want["inverted"] == False  # noqa: E712 (info[6] == 0)
    # the records of the run at the default tolerance: the twin's, to what the tolerance leaves
    assert np.array_equal(out["load"], want["load"]) and np.array_equal(out["probe_u"][-1], out["u"])
    early = want["residuals"] > 1e-8
    print(name, "residuals above 1e-8 against the twin's", rel(out["residuals"][early], want["residuals"][early]), "energies",
          rel(out["energies"], want["energies"]), "states", rel(out["probe_u"], want["states"]))
    assert rel(out["residuals"][early], want["residuals"][early]) <= 1e-6 and rel(out["energies"], want["energies"]) <= 1e-9
    assert rel(out["probe_u"], want["states"]) <= 2e-10 * ref / (lam_min * np.linalg.norm(u_star[~known]))
    # run on to the floor: converged under 4 FLOOR, u within the first-order bound of the twin's floor state
    bound = bar_r * ref / (lam_min * np.linalg.norm(u_star[~known]))
    err = rel(on["u"], u_star)
    rn = np.linalg.norm(np.where(known, 0.0, np.asarray(p.f_in) - hr.force(NH, *a, on["u"])[0])) / ref
    print(name, "run on: converged", on["converged"], "last residual", on["residuals"][-1], "bar", bar_r, "the twin's residual at the returned u", rn,
          "rel(u, u*)", err, "bound", bound)
    assert on["converged"] == 1 and on["residuals"][-1] <= bar_r
    assert err <= bound
    # f on P and the element rows against the twin's formulas at the device's own u
    fi = hr.neo_force(*a, on["u"], LD)[0]
    rows = hr.neo_element_rows(*a, on["u"], LD)
    f_err = float(np.abs((on["f"] - fi)[known]).max() / np.abs(fi).max())
    e_err = hr.rows_distance(on["elem"], rows)
    print(name, "f_out on P", f_err, "bar", 4 * SPREAD[name][0], "the element rows", e_err, "bar", 4 * SPREAD[name][3])
    assert f_err <= 4 * SPREAD[name][0] and e_err <= 4 * SPREAD[name][3]
    assert np.array_equal(on["f"][~known], np.asarray(p.f_in)[~known])


def test_newton_with_the_line_search(built):
    p = hr.case_problem("beam", "beam")
    want = hr.case_run(NH, "beam", "beam", 1, 8)
    with neo_context() as c:
        out = c.newton(p, increments=1, line_search=8)
    print("beam, one increment, line_search = 8: iterations", out["newton_iterations"], "halvings", out["halvings"], "step lengths", out["step_lengths"])
    assert list(out["newton_iterations"]) == list(want["newton_iterations"]) == [0, 10] and out["halvings"] == want["halvings"] == 2
    assert np.array_equal(out["step_lengths"], want["step_lengths"])


# ---- 5. mag_run_explicit, kinematics = "tl"
@functools.lru_cache(maxsize=None)
def explicit_exact(name, kind):
    s = tlc.setup(name, kind)
    p = s["prob"]
    return hr.explicit_tl(NH, *hr.of_problem(p), s["M"], s["free"], p.u_in, p.f_in, EXPLICIT_STEPS, tlc.dt_of(name, kind), s["alpha"], u0=s["u0"],
                          dtype=LD)


def explicit_run(c, name, kind, steps=EXPLICIT_STEPS, **kw):
    s = tlc.setup(name, kind)
    n2 = 2 * s["prob"].mesh.num_nodes
    kw.setdefault("u0", s["u0"])
    return c.explicit(steps=steps, dt=tlc.dt_of(name, kind), density=RHO, rayleigh=(s["alpha"], 0.0), probes=np.arange(n2), energies=True,
                      kinematics="tl", **kw)


def same_bits(a, b, what, skip=()):
    assert list(a) == list(b), what
    for k in a:
        if k not in skip:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


@pytest.mark.parametrize("name, kind", list(EXPLICIT_SPREAD))
def test_explicit_against_the_twin_fused_and_unfused(built, name, kind):
    s = tlc.setup(name, kind)
    p = s["prob"]
    known = np.asarray(p.u_known).reshape(-1) != 0
    want = explicit_exact(name, kind)
    s_u, s_v, s_a, s_f, s_e = EXPLICIT_SPREAD[(name, kind)]
    runs = {}
    for what, context in (("fused", {}), ("unfused", dict(op_variant=1))):
        with neo_context(**context) as c:
            c.upload_problem(p)
            out = runs[what] = explicit_run(c, name, kind)
            if what == "fused":
                again = explicit_run(c, name, kind)
        assert out["material"] == NH and out["fused"] == (1 if what == "fused" else 0) and not out["inverted"] and out["finite"] == 1
        err = {k: max(rel(out["probe_" + k][r], want[k][r]) for r in range(1, EXPLICIT_STEPS + 1)) for k in ("u", "v", "a")}
        err["f_P"] = rel(out["f"][known], want["f"][-1][known])
        err["energies"] = max(rel(out["energies"][:, k], want["energies"][:, k]) for k in range(3) if np.any(want["energies"][:, k]))
        print(name, kind, what, " ".join(f"{k} {v:.2e}" for k, v in err.items()), "bars", [4 * x for x in EXPLICIT_SPREAD[(name, kind)]])
        assert err["u"] <= 4 * s_u and err["v"] <= 4 * s_v and err["a"] <= 4 * s_a and err["f_P"] <= 4 * s_f and err["energies"] <= 4 * s_e
    same_bits(again, runs["fused"], "a repeat")
    print(name, kind, "fused against unfused: u", rel(runs["fused"]["u"], runs["unfused"]["u"]), "a", rel(runs["fused"]["a"], runs["unfused"]["a"]))
    assert rel(runs["fused"]["u"], runs["unfused"]["u"]) <= 8 * s_u and rel(runs["fused"]["a"], runs["unfused"]["a"]) <= 8 * s_a


def test_explicit_resumes_bit_for_bit_and_across_laws(built):
    name, kind, n1, n2 = "plate16", "pull5", 96, 160
    s = tlc.setup(name, kind)
    with neo_context() as c:
        c.upload_problem(s["prob"])
        whole = explicit_run(c, name, kind)
        explicit_run(c, name, kind, steps=n1)
        rest = explicit_run(c, name, kind, steps=n2, resume=True, u0=None)
        for k in ("u", "v", "a", "f"):
            assert rest[k].tobytes() == whole[k].tobytes(), k
        assert rest["probe_u"].tobytes() == whole["probe_u"][n1:].tobytes() and rest["resumed"] == 1
        # a St. Venant-Kirchhoff run resumed under neo-Hooke is accepted, and uses the law it finds
        c.set_material_law("svk")
        svk = explicit_run(c, name, kind, steps=n1)
        c.set_material_law(NH)
        mixed = explicit_run(c, name, kind, steps=n2, resume=True, u0=None)
        assert svk["material"] == "svk" and mixed["material"] == NH and mixed["resumed"] == 1 and mixed["finite"] == 1
        assert mixed["probe_u"][0].tobytes() == svk["u"].tobytes() and mixed["u"].tobytes() != whole["u"].tobytes()


# ---- 6. mag_run_transient_tl
@functools.lru_cache(maxsize=None)
def transient_setup(lumped):
    s = ttc.setup("beam", "beam", lumped, nominal=True)
    return s, s["T1"] / 20


@functools.lru_cache(maxsize=None)
def transient_twin(lumped, extra=0):
    s, dt = transient_setup(lumped)
    p = s["prob"]
    return hr.newmark_tl(NH, *hr.of_problem(p), s["M"], s["free"], p.u_in, p.f_in, TRANSIENT_STEPS, dt, newton_tol=1e-10, extra=extra)


@pytest.mark.parametrize("lumped", [False, True], ids=["consistent", "lumped"])
def test_transient_against_the_twin(built, lumped):
    s, dt = transient_setup(lumped)
    p = s["prob"]
    a = hr.of_problem(p)
    n2 = 2 * p.mesh.num_nodes
    known = np.asarray(p.u_known).reshape(-1) != 0
    free = np.flatnonzero(~known)
    want, floor = transient_twin(lumped), transient_twin(lumped, 4)
    bar_r = 4 * TRANSIENT_FLOOR[lumped]
    kw = dict(steps=TRANSIENT_STEPS, dt=dt, density=RHO, probes=np.arange(n2), energies=True, kinematics="tl", lumped=lumped)
    with neo_context() as c:
        out = c.transient(p, newton_tol=1e-10, cg_tol=1e-12, **kw)
        on = c.transient(newton_tol=bar_r, cg_tol=1e-13, **kw)
    print("transient beam", "lumped" if lumped else "consistent", "newton_iterations", out["newton_iterations"].tolist(), "the twin's",
          want["newton_iterations"].tolist(), "run on", on["newton_iterations"].tolist())
    assert out["material"] == NH and out["converged"] == 1 and not out["inverted"]
    assert np.array_equal(out["newton_iterations"], want["newton_iterations"])
    floors = [floor["residuals"][e - 3:e].max() for e in np.cumsum(floor["newton_iterations"][1:])]
    print("the twin's floor per step", floors, "FLOOR", TRANSIENT_FLOOR[lumped])
    # the first-order bound of a step: da <= 4 FLOOR ref / lambda_min(A_T,FF), carried over n steps
    c_u, c_v = 0.25 * dt * dt, 0.5 * dt
    A = (s["M"] + c_u * hr.tangent(NH, *a, floor["u"][-1]))[free][:, free].tocsc()
    lam_min = float(spla.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    fi = hr.force(NH, *a, floor["u"][-1])[0]
    mi = s["M"] @ floor["a"][-1]
    ref = max(np.linalg.norm(np.where(known, 0.0, p.f_in)), np.linalg.norm(fi[free]), np.linalg.norm(mi[free]))
    n = TRANSIENT_STEPS
    da = bar_r * ref / lam_min
    bars = dict(a=n * da / np.linalg.norm(floor["a"][-1]), v=n * c_v * da / np.linalg.norm(floor["v"][-1]),
                u=3 * n * n * c_u * da / np.linalg.norm(floor["u"][-1]))
    err = {k: rel(on[k], floor[k][-1]) for k in ("u", "v", "a")}
    err["f_P"] = rel(on["f"][known], floor["f"][-1][known])
    err["energies"] = max(rel(on["energies"][:, k], floor["energies"][:, k]) for k in range(3))
    print("run on: converged", on["converged"], " ".join(f"{k} {v:.2e}" for k, v in err.items()), "bars", bars)
    assert on["converged"] == 1 and on["newton_residuals"].reshape(-1)[np.cumsum(on["newton_iterations"][1:]) - 1].max() <= bar_r
    assert err["u"] <= bars["u"] and err["v"] <= bars["v"] and err["a"] <= bars["a"]
    assert err["f_P"] <= bars["a"] and err["energies"] <= 2 * max(bars["u"], bars["v"])  # (reactions: M a + f_int; energies: quadratic)
    rows = hr.neo_element_rows(*a, on["u"], LD)
    e_err = hr.rows_distance(on["elements"], rows)
    print("the element rows", e_err, "bar", 4 * SPREAD["beam"][3])
    assert e_err <= 4 * SPREAD["beam"][3]


# ---- 7. the law as context state
def three_passes(c, p):
    s = tlc.setup("plate16", "pull5")
    n = c.newton(p, increments=2)
    e = c.explicit(steps=16, density=RHO, u0=s["u0"], energies=True, kinematics="tl")
    t = c.transient(steps=3, dt=1e-5, density=RHO, energies=True, kinematics="tl")
    return n, e, t, c.internal_force(n["u"])[0], c.assemble_tangent(n["u"])


def test_the_default_is_svk_and_setting_it_back_gives_its_bits(built):
    p = tlc.setup("plate16", "pull5")["prob"]
    with Context(device=0) as c:
        assert c.material_law() == "svk"
        never = three_passes(c, p)
        c.set_material_law(NH)
        assert c.material_law() == NH
        neo = three_passes(c, p)
        c.set_material_law("svk")
        assert c.material_law() == "svk"
        back = three_passes(c, p)
    for k in range(3):
        same_bits(never[k], back[k], ("svk, never set against set back", k), skip=("message",))
        assert never[k]["material"] == "svk" and neo[k]["material"] == NH
        assert never[k]["u"].tobytes() != neo[k]["u"].tobytes()
    assert never[3].tobytes() == back[3].tobytes() and never[4].tobytes() == back[4].tobytes()
    assert never[3].tobytes() != neo[3].tobytes()


def test_the_law_survives_an_upload_and_leaves_the_other_results(built):
    s = tlc.setup("holes3k", "pull5")
    p = s["prob"]
    q = hr.case_problem("plate16", "load300")
    u_in = np.stack([p.u_in, 2.0 * p.u_in])
    f_in = np.stack([p.f_in, p.f_in])
    with Context(device=0) as c:
        c.upload_problem(p)
        c.run()
        run, cases_out, modal = c.download(), c.solve_cases(p, u_in, f_in), c.modal(modes=3, density=RHO)
        c.upload_problem(p)
        c.run()
        stored = c.newton(increments=1)
        stored_again = c.download_newton()
        c.set_material_law(NH)
        same_bits(c.download_newton(), stored_again, "a stored Newton run")
        for a, b in zip(run, c.download()):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        c.run()
        for a, b in zip(run, c.download()):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        again_cases, again_modal = c.solve_cases(p, u_in, f_in), c.modal(modes=3, density=RHO)
        for a, b in zip(cases_out, again_cases):
            for k in ("u", "f", "stress"):
                assert a[k].tobytes() == b[k].tobytes(), k
        for k in ("lambda", "frequency", "shapes"):
            assert again_modal[k].tobytes() == modal[k].tobytes(), k
        assert c.material_law() == NH
        c.upload_problem(q)
        assert c.material_law() == NH and c.newton(increments=2)["material"] == NH
        assert stored["material"] == "svk"


def test_refusals(built):
    p = hr.case_problem("plate16", "load300")
    half = meshgen.Problem(p.mesh, p.u_known, p.u_in, p.f_in, poisson_ratio=0.5)
    n2 = 2 * p.mesh.num_nodes
    with Context(device=0) as c:
        with pytest.raises(ValueError):
            c.set_material_law("mooney")
        assert c._L.mag_set_material_law(c._h, 2) == MAG_ERR_BAD_ARGS and b"mag_set_material_law: law = 2" in c._L.mag_last_error(c._h)
        assert c._L.mag_set_material_law(c._h, -1) == MAG_ERR_BAD_ARGS and c.material_law() == "svk"
        assert c._L.mag_get_material_law(c._h, None) == MAG_ERR_BAD_ARGS
        c.upload_problem(half)
        assert c.newton(increments=1)["converged"] == 1  # (nu = 0.5 under St. Venant-Kirchhoff is still accepted)
        c.set_material_law(NH)
        calls = (lambda: c.newton(increments=1), lambda: c.internal_force(np.zeros(n2)), lambda: c.assemble_tangent(np.zeros(n2)),
                 lambda: c.assemble_effective_tangent(np.zeros(n2), 1.0, 1.0, RHO), lambda: c.explicit(steps=2, density=RHO, kinematics="tl"),
                 lambda: c.transient(steps=2, dt=1e-5, density=RHO, kinematics="tl"))
        for call in calls:
            with pytest.raises(MagnetiteError, match="nu = 0.5") as e:
                call()
            assert e.value.code == MAG_ERR_BAD_ARGS
        assert c.explicit(steps=2, density=RHO)["finite"] == 1  # (the linear step reads no law)


def test_internal_force_reads_and_writes_device_memory(built):
    p = hr.case_problem("plate16", "load300")
    u = exact("plate16")[0]
    n2 = u.size
    with neo_context() as c:
        c.upload_problem(p)
        host_f, host_W, _ = c.internal_force(u)
        with DeviceArena() as arena:
            d_u, d_f = arena.put(u), arena.empty(n2)
            scalars = np.full(2, np.nan)
            rc = c._L.mag_internal_force(c._h, _dp(d_u.ptr), _dp(d_f.ptr), scalars.ctypes.data_as(C.POINTER(C.c_double)), MAG_MEM_DEVICE)
            assert rc == MAG_OK
            arena.check()
            got = arena.read(d_f)
    assert got.tobytes() == host_f.tobytes() and scalars[0] == host_W and scalars[1] == 0.0
