"""Every-entry checks of one solve's u, f and stress against the ORACLE's matrix (plain numpy + scipy; no GPU needed).

The sampled fixtures (tests/golden/fullsize_*.npz, roundoff_*.npz) look at 0.4 % of a million-entry result; a wrong last
block, one mis-permuted tile or one element read past a boundary moves no norm and is sampled only by luck.  These
helpers take K = oracle.assemble_sparse(...) -- the matrix the library's assembly is pinned to bit for bit -- and a
result (u, f, stress) from ANY solver, and look at all of it:

  residual()        |(f_in - K u)[free]| / |b|, the true residual under an operator that is not the solver's own.  One
                    wrong free entry of u shows here at the scale of a stiffness coefficient times the error.
  check_u()         prescribed entries bit-equal to the input, every entry finite.
  check_reactions() f off the prescribed DOFs bit-equal to the input; on them, row by row against K u within the
                    round-off of a dot product of that many terms: (terms + 2) * eps * (|K| |u|)_row, eps = 2^-53.
                    terms = the row's length when the reactions come from the assembled rows (the library's default),
                    6 * valence of the node when they come from the matrix-free operator (assemble_csr=0: 6 products
                    per incident triangle, never the summed coefficients).
  check_stress()    all E elements against oracle.stress() of the SAME u: the kernel claims the reference's order of
                    operations (no fused multiply-add, correctly rounded division and square root), so the bar is bit
                    equality, and the discontinuous `< 1.0` sign rule (solver.rs:524-530) needs no exclusion window.

Each check raises AssertionError and returns the figures it judged by (tests/test_fullsize_checks_cpu.py proves on the
CPU that each one passes on the oracle's own result and fails on single-entry mutations of it).
"""
import numpy as np

import oracle

EPS = 2.0 ** -53
TINY = np.finfo(float).tiny


class System:
    """The oracle's K of a meshgen.Problem with what the checks need of it, built once per workload."""

    def __init__(self, p, threads=8):
        import scipy.sparse as sp
        self.p = p
        self.K = oracle.assemble_sparse(p.xy_flat, p.conn_flat, p.poisson_ratio, p.youngs_modulus, p.part_thickness,
                                        threads=threads)
        self.known = p.u_known == 1
        _, b = oracle.reduce_system(self.K, p.u_known, p.u_in, p.f_in, threads=threads)
        self.b_norm = float(np.linalg.norm(b))
        self.absK = sp.csr_matrix((np.abs(self.K.val), self.K.col, self.K.rowptr), shape=(self.K.n, self.K.n))
        self.row_terms = np.diff(self.K.rowptr)
        self.apply_terms = np.repeat(6 * np.bincount(p.conn_flat, minlength=p.mesh.num_nodes), 2)

    def residual(self, u):
        """Relative true residual |b - K_ff x| / |b| of a full displacement vector (b = f_in - K_fk u_k on free rows)."""
        r = (self.p.f_in - self.K.spmv(u))[~self.known]
        return float(np.linalg.norm(r)) / self.b_norm

    def check_residual(self, u, bar):
        res = self.residual(u)
        assert res <= bar, f"true residual {res:.3e} of |b| above the bar {bar:.3e}"
        return res

    def check_u(self, u):
        assert u.shape == self.p.u_in.shape and np.all(np.isfinite(u)), "u has non-finite entries"
        assert np.array_equal(u[self.known], self.p.u_in[self.known]), "a prescribed displacement is not the input's bits"

    def reaction_ratios(self, u, f, matrix_free=False):
        """|f - K u| over its round-off bar, per prescribed DOF."""
        k = self.known
        terms = (self.apply_terms if matrix_free else self.row_terms)[k]
        bar = (terms + 2) * EPS * (self.absK @ np.abs(u))[k]
        return np.abs(f[k] - self.K.spmv(u)[k]) / np.maximum(bar, TINY)

    def check_reactions(self, u, f, matrix_free=False, ratio=None):
        """Returns the worst ratio of |f - K u| to its bar over the prescribed DOFs."""
        k = self.known
        assert f.shape == self.p.f_in.shape
        assert np.array_equal(f[~k], self.p.f_in[~k]), "f off the prescribed DOFs is not the input bit for bit"
        assert np.all(np.isfinite(f[k])), "a reaction is not finite"
        ratio = self.reaction_ratios(u, f, matrix_free) if ratio is None else ratio
        worst = int(np.argmax(ratio))
        assert ratio[worst] <= 1.0, (f"the reaction at prescribed DOF {np.flatnonzero(k)[worst]} is {ratio[worst]:.3g} x "
                                     f"its round-off bar away from the oracle's row product")
        return float(ratio[worst])

    def stress_differences(self, u, stress):
        """Elements whose stress is not, bit for bit, the oracle's arithmetic on the same u."""
        p = self.p
        ref = oracle.stress(p.xy_flat, p.conn_flat, u, p.poisson_ratio, p.youngs_modulus)
        assert stress.shape == ref.shape
        return np.flatnonzero(stress.view(np.uint64) != ref.view(np.uint64))

    def check_stress(self, u, stress, bad=None):
        """Bit equality with the oracle's arithmetic on the same u.  Returns the number of differing elements (0)."""
        bad = self.stress_differences(u, stress) if bad is None else bad
        assert bad.size == 0, (f"{bad.size} of {stress.size} element stresses differ from the oracle's on the same u, "
                               f"the first at element {bad[0]}: {stress[bad[0]]!r}")
        return int(bad.size)

    def check_all(self, u, f, stress, residual_bar, matrix_free=False, figures=None):
        """All of the above.  `figures` (a dict) receives each figure BEFORE it is judged, for the record."""
        fig = {} if figures is None else figures
        self.check_u(u)
        fig.update(true_residual=self.residual(u), residual_bar=residual_bar)
        assert fig["true_residual"] <= residual_bar, (f"true residual {fig['true_residual']:.3e} of |b| above the bar "
                                                      f"{residual_bar:.3e}")
        ratio = self.reaction_ratios(u, f, matrix_free)
        fig.update(reaction_ratio=float(ratio.max()))
        self.check_reactions(u, f, matrix_free, ratio)
        bad = self.stress_differences(u, stress)
        fig.update(stress_mismatches=int(bad.size))
        self.check_stress(u, stress, bad)
        return fig


def direct_solve(A, b, max_refine=10):
    """scipy splu (the options of tests/golden/make_roundoff_fixtures.py) + iterative refinement until the step stops
    shrinking, on an oracle Csr.  Returns x, its relative true residual and the relative size of the last step."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    lu = splu(sp.csr_matrix((A.val, A.col, A.rowptr), shape=(A.n, A.n)).tocsc(), permc_spec="MMD_AT_PLUS_A",
              diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    x = lu.solve(b)
    last = np.inf
    for _ in range(max_refine):
        dx = lu.solve(b - A.spmv(x))
        step = float(np.linalg.norm(dx) / np.linalg.norm(x))
        if step >= last:
            break
        x, last = x + dx, step
    return x, float(np.linalg.norm(b - A.spmv(x)) / np.linalg.norm(b)), last
