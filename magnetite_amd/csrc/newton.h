// Internal: launch wrappers of newton.hip (nonlinear statics, mag_run_newton and mag_assemble_tangent): the consistent tangent of
// explicit_tl.h's total-Lagrangian internal force in K's block-CSR pattern, and the small kernels of the Newton loop around it.
// Vectors are 2N in the caller's numbering.
//
// The tangent.  For a triangle (a, b, c) with tl_strain's H, F = I + H and S (explicit_tl.h):
//   reference shape gradients   g_a = (db.y - dc.y, dc.x - db.x) / 2A,  g_b = (dc.y, -dc.x) / 2A,  g_c = (-db.y, db.x) / 2A
//   V = A t,   D = c [[1, nu, 0], [nu, 1, 0], [0, 0, h]],   c = E / (1 - nu^2),   h = (1 - nu) / 2
//   the 2 x 2 block of corners (k, l):   K_T[k, l] = V (B_k^T D B_l + (g_k^T S g_l) I)
//   B_k (3 x 2), column d:   (F_d1 g_k.x,   F_d2 g_k.y,   F_d1 g_k.y + F_d2 g_k.x)
// With F = I and S = 0 this is the project's K.  In the kernel's constants (c0 = c t / 2, s = S / c): V c = 2A c0, and the block is
// 2A c0 (B_k^T (D / c) B_l + (g_k^T s g_l) I).
//
// The loop (api.hip, mag_run_newton).  Increment k under lambda = load[k]:  f_int(u)_F = lambda f_F,  u_P = lambda u_in.
//   first iteration    dU_P = lambda u_in - u on P;   K_T,FF du_F = (lambda f - f_int(u))_F - (K_T dU_P)_F;   u += s (du_F + dU_P)
//   later iterations   K_T,FF du_F = (lambda f - f_int(u))_F;   u += s du_F
//   stop               |r_F| <= newton_tol ref,   ref = max(|lambda f_F|, |f_int(u)_P|),   judged after every update
//   line search        Pi = W - lambda f_F.u_F;   slope g = (f_int(u) - lambda f_F).du (= -r.du where du_P = 0)
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "explicit_tl.h"
#include "transient.h"

namespace magk {

// kval[block (i, j)] = sum over the triangles that hold i and j, in the order of i's incidence list (mass_pattern's order), of
// K_T[i, j](u): kval's layout (4 doubles per block, the row's (k00, k01) pairs first, its (k10, k11) pairs behind them).  One lane
// per row node, no atomics but *inverted |= 1 for det F <= 0: the same bits for every grid and every tile size.  One launch.
void tl_tangent(const TlMesh &m, const Pattern &pat, const double *u, double *kval, int32_t *inverted, hipStream_t s);

// what the host reads of an evaluation: 56 bytes on the device
struct NewtonScalars {
    double W;        // the strain energy (tl_force)
    double r2;       // |(lambda f - f_int)_F|^2
    double f2, p2;   // |lambda f_F|^2, |f_int_P|^2: ref^2 is the larger
    double fu;       // f_F.u_F (Pi = W - lambda fu)
    double slope;    // (f_int - lambda f_F).du
    int32_t inverted, pad;
};

// the right-hand side of an iteration under lambda = load[at], a row walk over the pattern as pattern_apply's:
//   first != 0:  dup = lambda u_in - u on P, 0 on F;   rhs = known ? 0 : (lambda f - fint) - (K_T dup)
//   first == 0:  rhs = known ? 0 : lambda f - fint   (dup is not touched)
void newton_rhs(const Pattern &pat, const double *kval, const uint8_t *known, const double *f, const double *load, int64_t at,
                const double *fint, const double *u, const double *u_in, int32_t first, double *rhs, double *dup, hipStream_t s);

// out->r2, f2, p2, fu of the state u with its force fint under lambda = load[at]; with du also out->slope (else 0): the two-stage
// reduction of member_pass.h; partials: scratch [kSensBlocks][5].  Two launches.
void newton_norms(const uint8_t *known, const double *f, const double *load, int64_t at, const double *fint, const double *u,
                  const double *du, int64_t n2, double *partials, NewtonScalars *out, hipStream_t s);

// out = u + s du
void newton_update(const double *u, const double *du, double s, int64_t n2, double *out, hipStream_t s_);

// probe row `row` of u; with snap, u into it
void newton_record(const double *u, const int32_t *probes, int32_t num_probes, int64_t row, double *probe_u, double *snap, int64_t n2,
                   hipStream_t s);

// elem[e][8] = Exx, Eyy, Gxy, Sxx, Syy, Sxy, det F, W_e of the state u (cs = E / (1 - nu^2)); *inverted as tl_force
void newton_elements(const TlMesh &m, const double *u, double cs, double *elem, int32_t *inverted, hipStream_t s);

} // namespace magk
