"""The cases of the nonlinear transient tests (CPU and GPU), everything computed once, shared, left unchanged.

  every mesh of explicit_tl_cases.FOUR under load300, pull5 and pull5d: 8 steps, nominally at T1 / 20
  beam: 25 steps, nominally at T1 / 50 (half its first period: the tip moves 0.52 L)

T1 is the first period of the consistent-mass pencil (modal_ref.matrices(prob, RHO, False)).  The runs use the consistent mass
unless a test asks for the lumped one; pull5 / pull5d start from explicit_tl_cases' stretched u0, pull5d under its alpha.

The step of a case.  The GPU tests ask the device for the twin's Newton iteration counts, so a case is admitted only if every
step's last residual ratio is at most newton_tol / 10 and its last-but-one at least 10 newton_tol (tests/test_transient_tl.py).
Newton converges quadratically, so at the nominal steps some step of nearly every case lands an iterate between the two (plate16 /
load300 at T1 / 20: 2.4e-5 -> 8.0e-11; the beam at T1 / 50: 7.7e-4 -> 6.5e-10 -> floor).  The rule for that is to change the case's
dt, not the test: FACTOR scales the nominal step of each case to the nearest value of a scan over 0.1 .. 5 at which the case is
admitted with some room (the figures: last max, last-but-one min).  `nominal=True` gives the nominal step, for the CPU tests of the
method that compare with no device."""
import functools

import numpy as np

import explicit_tl_cases as tlc
import modal_ref
import newton_ref
import transient_ref
import transient_tl_ref as ref

RHO = tlc.RHO
FOUR = tlc.FOUR
KINDS = tlc.KINDS
CASES = tlc.CASES
NEWTON_TOL = 1e-10
CG_TOL = 1e-12
FACTOR = {
    ("plate16", "load300"): 0.6,     # 3.0e-12, 3.2e-9
    ("holes3k", "load300"): 0.46,    # 9.0e-12, 1.15e-9
    ("frontal3k", "load300"): 0.45,  # 7.3e-12, 1.27e-9
    ("two_fans", "load300"): 0.2,    # 8.1e-12, 1.39e-9
    ("plate16", "pull5"): 0.2,       # 2.1e-12, 4.4e-7
    ("holes3k", "pull5"): 0.25,      # 6.6e-12, 1.38e-9
    ("frontal3k", "pull5"): 1.8,     # 4.2e-13, 1.5e-9
    ("two_fans", "pull5"): 1.8,      # 4.5e-13, 2.3e-9
    ("plate16", "pull5d"): 0.2,      # 2.1e-12, 4.2e-7
    ("holes3k", "pull5d"): 0.25,     # 6.5e-12, 1.38e-9
    ("frontal3k", "pull5d"): 1.8,    # 5.0e-13, 1.31e-9
    ("two_fans", "pull5d"): 1.8,     # 4.3e-13, 1.93e-9
    ("beam", "beam"): 0.35,          # 3.1e-12, 6.6e-6
}


@functools.lru_cache(maxsize=None)
def setup(name, kind, lumped=False, nominal=False):
    """dict(prob, K, M, free, alpha, u0, T1, steps, dt): explicit_tl_cases' problem with the mass asked for"""
    s = tlc.setup(name, kind)
    prob = s["prob"]
    K, Mc, free = modal_ref.matrices(prob, RHO, False)
    lam, _ = modal_ref.eigenpairs(K, Mc, free, k=1)
    T1 = 2.0 * np.pi / np.sqrt(float(lam[0]))
    M = modal_ref.matrices(prob, RHO, True)[1] if lumped else Mc
    steps, div = (25, 50) if kind == "beam" else (8, 20)
    dt = T1 / div * (1.0 if nominal else FACTOR[(name, kind)])
    return dict(prob=prob, K=K, M=M, free=free, alpha=s["alpha"], u0=s["u0"], T1=T1, steps=steps, dt=dt)


@functools.lru_cache(maxsize=None)
def twin(name, kind, extra=0, lumped=False, steps=None, dt=None, newton_tol=NEWTON_TOL, max_newton=0):
    """the twin's run of a case (extra=3: on to its round-off floor)"""
    s = setup(name, kind, lumped)
    p = s["prob"]
    return ref.newmark_tl(*ref.of_problem(p), s["M"], s["free"], p.u_in, p.f_in, s["steps"] if steps is None else steps,
                          s["dt"] if dt is None else dt, alpha=s["alpha"], u0=s["u0"], newton_tol=newton_tol, max_newton=max_newton,
                          extra=extra)


# ---- the cases of the paths the first suite only brushed (tests/test_transient_tl_paths_gpu.py), admitted like the ones above
# in tests/test_transient_tl.py.  The figures: the converged steps' last max and last-but-one min; the ratio at the cap.
# The jump was scanned like FACTOR.  A single level of 20 (the issue's starting point) is not admitted at the cap of 6: step 4 ends
# at 3.2e-11 > newton_tol / 10, and under every level from 15 to 19.8 step 5's last-but-one is below 10 newton_tol.  Two levels are.
JUMP_AT = 4
EARLY = dict(jump_to=18.0, jump_then=24.0, max_newton=5)  # 3 steps (5, 4, 4), step 4 at 2.1e-6 at the cap; 2.4e-12, 3.4e-9
LONG = dict(jump_to=18.0, jump_then=24.0, max_newton=6)   # all 8 steps ([0 5 4 4 6 5 4 4 4]); 2.4e-12, 2.9e-9
INVERTED = dict(jump_to=100.0, max_newton=5)              # 3 steps, step 4 at 0.20 at the cap, a trial's smallest det F -4.6
NEWMARK = [                                   # (name, kind, beta, gamma, lumped)
    ("plate16", "pull5d", 0.3025, 0.6, False),   # 1.0e-12, 1.9e-7
    ("plate16", "pull5d", 0.5, 1.0, False),      # 1.2e-13, 2.4e-8
    ("plate16", "load300", 0.5, 1.0, False),     # 2.9e-12, 3.6e-9
    ("plate16", "pull5d", 0.5, 1.0, True),       # 1.3e-13, 2.5e-8
]


def jump(to, then=None, steps=8):
    """the amplitude of the early-end cases: 1, 1.01, 1.02, 1.03 (no two rows alike: a row taken for its neighbour shows), `to` at
    row JUMP_AT, `then` (None: `to`) behind it"""
    amp = 1.0 + 0.01 * np.arange(steps + 1)
    amp[JUMP_AT] = to
    amp[JUMP_AT + 1:] = to if then is None else then
    return amp


@functools.lru_cache(maxsize=None)
def twin_with(name, kind, extra=0, lumped=False, steps=None, max_newton=0, beta=0.25, gamma=0.5, jump_to=None, jump_then=None, definite=False):
    """the twin's run of a case under other Newmark parameters or the amplitude jump(jump_to, jump_then); definite=True: with
    out["definite"], the smallest ratio of smallest to largest eigenvalue over the matrices the run factors"""
    s = setup(name, kind, lumped)
    p = s["prob"]
    steps = s["steps"] if steps is None else steps
    ratios = []
    out = ref.newmark_tl(*ref.of_problem(p), s["M"], s["free"], p.u_in, p.f_in, steps, s["dt"], beta=beta, gamma=gamma, alpha=s["alpha"],
                         amplitude=None if jump_to is None else jump(jump_to, jump_then)[:steps + 1], u0=s["u0"], newton_tol=NEWTON_TOL,
                         max_newton=max_newton, extra=extra,
                         on_factor=(lambda A: ratios.append(newton_ref.definiteness(A))) if definite else None)
    if definite:
        out["definite"] = min(ratios)
    return out


@functools.lru_cache(maxsize=None)
def linear(name, kind, steps=None, dt=None):
    """the linear Newmark twin's run of a case"""
    s = setup(name, kind)
    p = s["prob"]
    return transient_ref.newmark(s["K"], s["M"], s["free"], p.u_in, p.f_in, s["steps"] if steps is None else steps,
                                 s["dt"] if dt is None else dt, alpha=s["alpha"], u0=s["u0"])


def rel(a, b):
    """|a - b| / |b| (0 / 0 = 0)"""
    n = float(np.linalg.norm(np.asarray(b)))
    d = float(np.linalg.norm(np.asarray(a) - np.asarray(b)))
    return d / n if n > 0 else d
