"""GPU: mag_run_modal at every shape of its kernels and on the parts where its Rayleigh-Ritz step used to refuse legal input.

- every subspace shape: each instantiation of k_modal_rotate (QC = 8 / 16 / 24 / 32) at its upper limit and at the first q above
  the previous one, the Gram tails q mod 4 = 1, 2, 3, 0, R written for modes == q and modes < q, on one tile and on several;
- the rotation's R, the Gram tail and the norm kernels pinned numerically: the pass's own residual against the true one after
  two outer steps, where the residuals are large;
- slender parts and wide subspaces, a strip one element thick, a clustered spectrum;
- the error returns, which leave the context whole.

The bars are those of check_modes (tests/test_modal_gpu.py): eigenvalues 1e-8, |Phi^T M Phi - I| 1e-10, true residual 1e-4,
1 - MAC 1e-8 on modes 1-4, zero on supports, the sign rule, the frequency identity.  The outer steps are measured against the
numpy prototype of tests/modal_ref.py with the same (p, q, tol), the same start vectors and sparse LU inner solves:
outer <= prototype + max(2, prototype // 4), the margin for the CG inner solves."""
import functools

import numpy as np
import pytest

import modal_ref as ref
from magnetite_amd import Context, meshgen
from magnetite_amd.solver import MagnetiteError
from test_modal_gpu import MAG_ERR_STATE, RHO, assert_same_bits, check_modes

pytestmark = pytest.mark.gpu

MAG_ERR_NOT_CONVERGED = 3
SHAPES = ((1, 1), (1, 2), (3, 3), (4, 8), (6, 9), (8, 16), (9, 17), (12, 24), (17, 25), (16, 32), (24, 32))
MAX_OUTER = 50


def pairs(p):
    """reference pairs for p modes: at least p + 1 (check_modes wants one more than it compares)"""
    return max(8, p + 1)


@functools.lru_cache(maxsize=None)
def prototype(name, p, q):
    """the numpy prototype on part `name` with exact inner solves: computed once per (part, shape), left unchanged"""
    prob, K, M, free, _, _ = ref.cached(name, RHO, False, pairs(p))
    return ref.subspace_iteration(K, M, free, ref.start_vectors(prob.mesh.xy, prob.u_known, q), p, tol=1e-10, max_outer=MAX_OUTER)


def run_and_check(name, p, q=0, **ctx_opts):
    """modal() on part `name`, every bar of check_modes, the outer rule; returns (out, the largest CG iteration count of the last step)"""
    prob = ref.PARTS[name]()
    with Context(device=0, **ctx_opts) as c:
        out = c.modal(prob, modes=p, subspace=q, density=RHO, max_outer=MAX_OUTER)
        iterations = max(c.modal_stats(j)["iterations"] for j in range(out["subspace"]))
    proto = prototype(name, p, out["subspace"])
    print(name, (p, out["subspace"]), "outer", out["outer"], "prototype", proto["outer"], "prototype's smallest pivot figure",
          min(proto["pivots"]), "CG iterations of the last step (largest)", iterations)
    check_modes(name, out, max_outer=MAX_OUTER, pairs=pairs(p))
    assert proto["converged"] == 1 and proto["refused"] == 0
    assert out["converged"] == 1 and out["outer"] <= proto["outer"] + max(2, proto["outer"] // 4), (out["outer"], proto["outer"])
    return out, iterations


# ---- A1: every subspace shape

@pytest.mark.parametrize("p,q", SHAPES)
def test_every_subspace_shape_on_one_tile(built, p, q):
    out, _ = run_and_check("plate16", p, q)
    assert out["modes"] == p and out["subspace"] == q


@pytest.mark.parametrize("p,q", [(9, 17), (17, 25), (24, 32)])
def test_the_wide_shapes_on_several_tiles(built, p, q):
    out, _ = run_and_check("holes3k", p, q)
    assert out["modes"] == p and out["subspace"] == q


# ---- A2: the pass's own residual against the true one

@pytest.mark.parametrize("p,q", SHAPES)
def test_own_residual_equals_the_true_residual_after_two_steps(built, p, q):
    """After two outer steps nothing has converged and the residuals are large, so that the pass's own figure -- R of
    k_modal_rotate, the tail of the Gram stage through lambda and Q, k_modal_norm_* -- is pinned by its value, not by "small".

    r_own - r_true = (Y_old - K Z) Q: the inner solves leave |Y_old_j - K z_j| <= cg_tol |Y_old_j|, so the two relative residuals
    differ by at most cg_tol * sum_j |Q_jk| |Y_j| / |lambda_k M phi_k|, of order 1e-12 * q * lambda_q / lambda_1 ~ 1e-8 here.
    The bar is 1e-6 absolute: 100 x that bound, and orders below the residuals themselves.  A dropped tail column, a wrong
    zero-fill past q or a wrong lambda[k] moves the residual by its own size."""
    prob, K, M, free, _, _ = ref.cached("plate16", RHO, False, pairs(p))
    with Context(device=0) as c:
        out = c.modal(prob, modes=p, subspace=q, density=RHO, max_outer=2, cg_tol=1e-12)
    shapes = out["shapes"]
    true = np.array([ref.true_residual(K, M, free, out["lambda"][k], shapes[k]) for k in range(p)])
    ortho = float(np.max(np.abs(shapes @ (M @ shapes.T) - np.eye(p))))
    print((p, q), "own residual", out["residual"], "true residual", true, "largest difference", float(np.max(np.abs(out["residual"] - true))),
          "ortho", ortho)
    assert out["converged"] == 0 and out["outer"] == 2
    assert np.all(np.isfinite(shapes)) and out["residual"].shape == (p,)
    assert np.max(np.abs(out["residual"] - true)) <= 1e-6
    assert ortho <= 1e-10
    assert np.all(out["lambda"] > 0) and np.all(np.diff(out["lambda"]) >= 0)


@pytest.mark.parametrize("name", ["plate16", "holes3k"])
def test_the_first_step_is_the_prototypes(built, name):
    """The Ritz values after ONE outer step are those of the prototype: k_modal_start is the twin of modal_ref.hash_unit and the
    host's Rayleigh-Ritz step that of modal_ref.rayleigh_ritz (different start vectors, or a different pencil, give different
    values in the first digit: nothing has converged).  The inner solves differ -- CG to cg_tol = 1e-12 against sparse LU --
    by cg_tol relative in K z, which a Ritz value sees magnified by at most q lambda_q / lambda_1 ~ 12 * 40: 5e-10.  Bar 5e-8,
    100 x that."""
    prob, K, M, free, _, _ = ref.cached(name, RHO, False, 8)
    proto = ref.subspace_iteration(K, M, free, ref.start_vectors(prob.mesh.xy, prob.u_known, 12), 6, max_outer=1)
    with Context(device=0) as c:
        out = c.modal(prob, modes=6, density=RHO, max_outer=1, cg_tol=1e-12)
    diff = np.abs(out["lambda"] - proto["lam"]) / proto["lam"]
    print(name, "Ritz values after step 1", out["lambda"], "prototype", proto["lam"], "relative difference", diff)
    assert out["outer"] == 1 and out["converged"] == 0
    assert np.max(diff) <= 5e-8


# ---- A3: slender parts and wide subspaces

@pytest.mark.parametrize("name,p", [("beam16", 6), ("beam8", 6), ("beam8", 12), ("bar4", 20), ("plate16", 24), ("frontal3k", 24)])
def test_slender_parts_and_wide_subspaces(built, name, p):
    """Cantilevers (left edge fixed) of 16:1, 8:1 and 4:1 and the widest default subspaces.  With the Cholesky factor of
    Z^T M Z and monomial start vectors -- the first version -- the prototype with exact solves puts the smallest pivot of step 1,
    as a fraction of the largest diagonal entry and refused at 1e-13, at 1.4e-14 (beam16: refused at column 9), 1.2e-13
    (beam8, q = 12), 7.0e-14 (beam8, q = 20: refused at column 11), 9.0e-14 (bar4: refused at column 19), 1.2e-13 (plate16)
    and 2.8e-13 (frontal3k): three refusals and three that CG's 1e-10 decides.  The device agreed: beam16, beam8 (12, 20) and
    bar4 came back "outer step 1: the vectors of the subspace are linearly dependent (pivot 9 / 11 / 19 of Z^T M Z)", the other
    three passed.

    The prototype of modal_ref alone, exact inner solves, on the CPU (part, (p, q): eigenvalue error, orthogonality, true
    residual, 1 - MAC, outer steps, smallest pivot figure) -- each at least 10 x inside its bar:
      beam16    (6, 12):  2.0e-13  1.9e-15  1.2e-06  1.1e-16   7  1.9e-05
      beam8     (6, 12):  9.3e-14  3.6e-15  7.3e-07  1.0e-15   8  3.0e-05
      beam8     (12, 20): 5.2e-12  2.4e-15  3.2e-06  3.3e-16  12  1.4e-05
      bar4      (20, 28): 5.0e-11  6.7e-15  5.6e-06  6.7e-16  26  7.0e-05
      plate16   (24, 32): 7.3e-11  3.3e-15  4.9e-06  5.6e-16  39  1.7e-03
      frontal3k (24, 32): 1.2e-10  2.1e-15  5.8e-06  4.4e-16  35  1.2e-03"""
    out, iterations = run_and_check(name, p, max_iter=100000)
    assert out["subspace"] == min(2 * p, p + 8)
    assert 0 < iterations < 100000


def test_a_strip_one_element_thick(built):
    """plate(32, 1, lx=8, ly=0.25): eta takes two values, so polynomial start vectors with eta^2 are exactly dependent (the
    first version: refused at column 5 of step 1, pivot 4e-14 of the largest diagonal entry, on the device as in the
    prototype).  The start vectors are a hash of the coordinates now and are independent on any mesh: the strip solves to the bars (prototype
    alone: 3.7e-13, 2.2e-15, 1.8e-06, 7.8e-16, 7 outer steps, smallest pivot figure 1.7e-05)."""
    out, _ = run_and_check("strip", 6, max_iter=100000)
    assert out["subspace"] == 12


# ---- A4: a clustered spectrum

@pytest.mark.parametrize("p,q", [(6, 12), (3, 3)])
def test_a_clustered_spectrum(built, p, q):
    """plate(16) with every boundary node clamped: lambda_2 / lambda_1 = 1.016 and modes 5-7 a triple at 2.77 / 2.81 / 2.87
    lambda_1, which p = 6 cuts (prototype alone: 18 / 26 outer steps, eigenvalue error <= 4.2e-11, 1 - MAC <= 4.1e-11)."""
    lam = ref.cached("clamped16", RHO, False, pairs(p))[4]
    assert lam[1] / lam[0] < 1.02 and lam[6] / lam[4] < 1.05  # the part is what the test says it is
    run_and_check("clamped16", p, q)


# ---- A5: error returns leave the context whole

def test_an_unsupported_part_is_an_error_and_the_context_stays_usable(built):
    mesh = meshgen.plate(8)
    n2 = 2 * mesh.num_nodes
    floating = meshgen.Problem(mesh, np.zeros(n2, dtype=np.uint8), np.zeros(n2), np.zeros(n2))
    plate16 = ref.PARTS["plate16"]()
    with Context(device=0, max_iter=200) as c:
        c.upload_problem(floating)
        with pytest.raises(MagnetiteError) as e:
            c.modal(modes=2, density=RHO)
        print("unsupported part:", e.value.code, e.value.message)
        assert e.value.code == MAG_ERR_NOT_CONVERGED  # (the inner solve's own status: the cap or a breakdown, both this code)
        assert "mag_run_modal" in e.value.message
        with pytest.raises(MagnetiteError) as e:
            c.download_modal()
        assert e.value.code == MAG_ERR_STATE
        after = c.modal(plate16, modes=6, density=RHO)
    with Context(device=0, max_iter=200) as fresh:
        want = fresh.modal(plate16, modes=6, density=RHO)
    assert after["converged"] == 1
    assert_same_bits(after, want, "after the refusal")


def test_no_guard_vectors_and_a_low_cap(built):
    prob, K, M, free, _, _ = ref.cached("plate16", RHO, False, 8)
    with Context(device=0) as c:
        out = c.modal(prob, modes=32, subspace=32, density=RHO, max_outer=3)
    shapes = out["shapes"]
    assert out["converged"] == 0 and out["outer"] == 3 and out["modes"] == 32 and shapes.shape == (32, 2 * prob.mesh.num_nodes)
    assert np.all(np.isfinite(shapes))
    assert np.all(out["lambda"] > 0) and np.all(np.diff(out["lambda"]) >= 0)
    assert np.max(np.abs(shapes @ (M @ shapes.T) - np.eye(32))) <= 1e-10
