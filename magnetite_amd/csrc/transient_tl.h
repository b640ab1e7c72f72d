// Internal: launch wrappers of transient_tl.hip (nonlinear transient dynamics, mag_run_transient_tl and
// mag_assemble_effective_tangent): Newmark's method in acceleration form on explicit_tl.h's total-Lagrangian internal force,
// every step solved by Newton's method on newton.h's consistent tangent.  Vectors are 2N in the caller's numbering.
//
// The method.  Supports, loads, start, mass and records are transient.h's: u_P = u_in, v_P = a_P = 0; the load on F is
// amplitude[n] f_in; the mass is consistent or lumped; C = alpha M (no stiffness-proportional term, as under explicit TL).
//   start   M_FF a_0 = (amp[0] f - alpha M v_0 - f_int(u_0))_F
//   step    ut = u + dt v + dt^2 (1/2 - beta) a,   vt = v + dt (1 - gamma) a      (on P: ut = u_in, vt = 0)
//           unknown a':  u' = ut + beta dt^2 a',   v' = vt + gamma dt a'
//           r(a')   = (amp[n+1] f - f_int(u') - M (a' + alpha v'))_F
//           Newton:  A_T,FF da = r_F,   A_T = (1 + gamma dt alpha) M + beta dt^2 K_T(u'),   a' += da
//           first iterate:  a'_F = (u - ut)_F / (beta dt^2), so that u' = u_n (zero displacement increment; a' = a_n or a' = 0
//                    rotate the part linearly, stretch it, and Newton diverges at the steps the pass is for)
//           stop, judged after every update:  |r_F| <= newton_tol * ref
//                    ref = max(|amp[n+1] f_F|, |f_int(u')_F|, |(M (a' + alpha v'))_F|)
//   reactions   f_int(u) + M (a + alpha v) on P,  amp[n] f on F
//   energies    T = 1/2 v.Mv,  W = the elements' strain energies,  P = amp[n] f_F.u_F
// The start is the residual with a' = 0, v' = v_0 and a solve on M alone (transient.h's effective_values with (c_M, c_K) = (1, 0)).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "newton.h"

namespace magk {

// aval = c_K K_T(u) + c_M M in kval's layout, one launch: tl_tangent's row walk (one lane per row node, incidence-list order, no
// floating-point atomics), the lane finishing its row with effective_values's expression on mval.  Bit for bit
// effective_values(tl_tangent(u), mval, c_K, c_M); only aval is written.  *inverted |= 1 for det F <= 0
void tl_effective_tangent(const TlMesh &m, const Pattern &pat, const double *u, const double *mval, double c_K, double c_M, double *aval,
                          int32_t *inverted, hipStream_t s);

// the trial state of a Newton iteration, one launch:
//   first == 0:  an = a_it + s da;   first != 0:  an = (u - ut) / c_u on F, 0 on P   (the first iterate: u' = u_n)
//   un = ut + c_u an,   vn = vt + c_v an        (c_u = beta dt^2, c_v = gamma dt; an may be a_it)
struct TlTrial {
    int64_t n2;
    const uint8_t *known;
    const double *u, *ut, *vt; // the step's state and predictors
    const double *a_it, *da;
    double *an, *un, *vn;
};
void tl_trial_state(const TlTrial &t, double s_len, double c_u, double c_v, int32_t first, hipStream_t s);

// what the host reads of a Newton iteration: 40 bytes on the device
struct TlStepScalars {
    double r2;         // |r_F|^2
    double f2, i2, m2; // |amp f_F|^2, |f_int_F|^2, |(M (a' + alpha v'))_F|^2: ref^2 is the largest
    int32_t inverted, pad;
};

// r = known ? 0 : amplitude[amp_at] f - fint - M (a + alpha v), one row walk over mval (a row in ascending column order), and the
// four sums of TlStepScalars of it: stage one in the same launch (each lane its fixed share of the rows), member_pass.h's second
// stage behind it.  partials: scratch [kSensBlocks][4].  Two launches
void tl_residual(const Pattern &pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude, int64_t amp_at,
                 const double *fint, const double *a, const double *v, double alpha, double *r, double *partials, TlStepScalars *out,
                 hipStream_t s);

// the reactions: out = fint + M (a + alpha v) on P, amplitude[amp_at] f on F
void tl_dynamic_reactions(const Pattern &pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude,
                          int64_t amp_at, const double *fint, const double *a, const double *v, double alpha, double *out, hipStream_t s);

// an energy row: out[0] = 1/2 v.Mv (the row walk over mval), out[1] = W(u) over the elements, out[2] = amplitude[amp_at] f.u_F;
// partials: scratch [kSensBlocks][3].  Two launches; *inverted as tl_force
void tl_dynamic_energies(const TlMesh &m, const Pattern &pat, const double *mval, const uint8_t *known, const double *u, const double *v,
                         const double *f, const double *amplitude, int64_t amp_at, int32_t *inverted, double *partials, double *out,
                         hipStream_t s);

} // namespace magk
