// Internal: launch wrappers of transient.hip (transient dynamics, mag_run_transient: the consistent or lumped mass in K's
// block-CSR pattern, the effective matrix A = c_K K + c_M M, y = K x1 + M x2 over the block rows, the fused vector updates of
// Newmark's method and its records).  Vectors are 2N in the caller's numbering.
//
// The method (Newmark in acceleration form; beta, gamma taken literally).  F: DOFs with u_known == 0, P: the supports, held at
// the uploaded u_in for all time (u_P = u_in, v_P = a_P = 0).  C = alpha M + eta K.  The load on F is amplitude[n] f_in.
//   start:  M_FF a_0 = (amplitude[0] f - C v_0 - K u_0)_F
//   step:   ut = u + dt v + dt^2 (1/2 - beta) a,   vt = v + dt (1 - gamma) a
//           A_FF a' = (amplitude[n+1] f - alpha M vt - K (ut + eta vt))_F,  A = (1 + gamma dt alpha) M + (beta dt^2 + gamma dt eta) K
//           u' = ut + beta dt^2 a',   v' = vt + gamma dt a'
// Both solves are one code with other coefficients ((c_M, c_K) = (1, 0) for a_0).  Prescribed displacements enter through
// K ut (ut_P = u_in): there is no elimination pass.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace magk {

// K's block-CSR pattern of the uploaded mesh (caller numbering): row node i holds blocks bptr[i] .. bptr[i + 1], columns bcol
// ascending; kval: 4 doubles per block, the row's (k00, k01) pairs first, its (k10, k11) pairs behind them; mval: one per block
struct Pattern {
    const int32_t *bptr, *bcol;
    int64_t N, nb;
};

// the diagonal entry of mval in row node i: the lumped mass of node i
__device__ inline double diagonal_mass(const Pattern &pat, const double *mval, int64_t i)
{
    double m = 0.0;
    for (int32_t p = pat.bptr[i]; p < pat.bptr[i + 1]; ++p)
        if (pat.bcol[p] == i) m = mval[p];
    return m;
}

// mval[block (i, j)] = sum over the triangles that hold i and j, in the order of i's incidence list (inc_off / inc by Hilbert
// position, inc = 3 e + corner), of m_e / 12 (i != j) or m_e / 6 (i == j), m_e = c |A_e|, c = rho t; lumped: m_e / 3 on the
// diagonal, 0 elsewhere.  One launch.
void mass_pattern(const Pattern &pat, const uint32_t *perm, const int32_t *inc_off, const uint32_t *inc, const int32_t *conn,
                  const double *xy, double c, int32_t lumped, double *mval, hipStream_t s);

// aval = c_K kval + c_M mval I in kval's layout; kval is read only
void effective_values(const Pattern &pat, const double *kval, const double *mval, double c_K, double c_M, double *aval, hipStream_t s);

// y = K x1 + M x2 with x1 = ca xa + cb xb and x2 = cc xc + cd xd (a null vector drops its term), one thread per DOF, the row in
// ascending column order, K's sum first.  What is stored:
//   kind 0: y;   kind 1 (right-hand side): known ? 0 : amp f - y;   kind 2 (reactions): known ? y : amp f
// with amp = amplitude[amp_at] read on the device.  With ku / mv (energies) also ku = K xa and mv = M xc.
struct PatternApply {
    const double *kval, *mval;
    const double *xa, *xb, *xc, *xd;
    double ca, cb, cc, cd;
    int32_t kind;
    const uint8_t *known;
    const double *f, *amplitude;
    int64_t amp_at;
    double *y, *ku, *mv;
};
void pattern_apply(const Pattern &pat, const PatternApply &a, hipStream_t s);

// the state of the time loop and the records of one run, all on the device
struct NewmarkState {
    int64_t n2;         // 2N
    double *u, *v, *a;  // the state
    double *ut, *vt;    // the predictors
    const uint8_t *known;
    const double *u_in;
    int32_t num_probes;
    const int32_t *probes;                // DOF indices, caller numbering
    double *probe_u, *probe_v, *probe_a;  // [rows][num_probes]
};

// ut = u + dt v + dt^2 (1/2 - beta) a, vt = v + dt (1 - gamma) a; on P: ut = u_in, vt = 0
void newmark_predict(const NewmarkState &st, double dt, double beta, double gamma, hipStream_t s);
// u = ut + beta dt^2 a, v = vt + gamma dt a (a: the step's solution, 0 on P); probe row `row`; with snap, u into it
void newmark_correct(const NewmarkState &st, double dt, double beta, double gamma, int64_t row, double *snap, hipStream_t s);
// probe row `row` and the snapshot of the state as it is (row 0 of a run)
void newmark_record(const NewmarkState &st, int64_t row, double *snap, hipStream_t s);
// the start: u = u0 (or 0) on F, u_in on P; v = v0 (or 0) on F, 0 on P; a = 0
void newmark_start(const NewmarkState &st, const double *u0, const double *v0, hipStream_t s);

// out[0..2] = T = 1/2 v.mv, W = 1/2 u.ku, P = amplitude[amp_at] sum over F of f u: the two-stage reduction of member_pass.h;
// partials: scratch [kSensBlocks][3].  Two launches.
void newmark_energies(const NewmarkState &st, const double *ku, const double *mv, const double *f, const double *amplitude,
                      int64_t amp_at, double *partials, double *out, hipStream_t s);

// b[fidx[d]] = x[d] for the free DOFs d (fidx: the exclusive scan of the free flags): a caller-numbered vector in the compact
// numbering of the CSR operator's phase
void compact_free(const double *x, const int32_t *fidx, const uint8_t *known, int64_t n2, double *b, hipStream_t s);

// *bad = the first probe outside [0, n2) (all ones: none)
void check_probes(const int32_t *probes, int32_t num_probes, int64_t n2, unsigned long long *bad, hipStream_t s);

} // namespace magk
