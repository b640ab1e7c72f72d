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
// Under kLawNeoHooke (explicit_tl.h) the material tangent is 2 dS/dC = 2 mu C33 (kappa C^-1 (x) C^-1 + I_{C^-1}) with
// kappa = Lambda / (2 mu C33 + Lambda).  Put through B_k^T DD B_l + (g_k^T S g_l) I, the (h_k . h_l) I terms of the material and the
// geometric part cancel, h_k = F^-T g_k being the spatial gradient, and the block is
//   K_T[k, l] = V (mu (g_k . g_l) I + mu C33 (2 kappa h_k h_l^T + h_l h_k^T))
// The kernel uses this compact form (the tests' twin the B^T DD B form): in its constants (c0 = mu t / 2, lr = Lambda / mu)
// V mu = 2A c0 and kappa = lr / (2 C33 + lr).  K_T[l, k] = K_T[k, l]^T; at u = 0 it is the project's K (2 mu kappa is the
// plane-stress lambda).  F^-T divides by det F: an element with det F = 0 gives non-finite entries, which the CG's finite check
// catches; one with det F < 0 finite ones.
//
// The loop (api.hip, mag_run_newton).  Increment k under lambda = load[k]:  f_int(u)_F = lambda f_F,  u_P = lambda u_in.
//   first iteration    dU_P = lambda u_in - u on P;   K_T,FF du_F = (lambda f - f_int(u))_F - (K_T dU_P)_F;   u += s (du_F + dU_P)
//   later iterations   K_T,FF du_F = (lambda f - f_int(u))_F;   u += s du_F
//                      (behind a step with s < 1 the supports are short of lambda u_in: a first iteration again, on the rest)
//   stop               |r_F| <= newton_tol ref,   ref = max(|lambda f_F|, |f_int(u)_P|),   judged after every update (supports in place)
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

// The tangent's row of the node at Hilbert position g (caller id perm[g]), by the one lane that owns it: the row's values are
// zeroed, then every incident triangle adds its three blocks of this node's row, in list order.  The triangle is always taken
// from its first corner on, so that its three rows see the same H, F and S.  EFFECTIVE (transient_tl.hip): the lane then finishes
// the row in place with effective_values's expression, val = c_K val + c_M mval on the blocks' diagonals -- no K_T is kept.
template <int LAW, bool EFFECTIVE>
__device__ inline void tl_tangent_row(const TlMesh &m, const Pattern &pat, const double2 *u, int64_t g, double *val, int32_t *inverted,
                                      const double *mval, double c_K, double c_M)
{
    const int64_t i = m.perm[g];
    const int32_t p = pat.bptr[i], cnt = pat.bptr[i + 1] - p;
    double *row0 = val + 4 * (int64_t)p, *row1 = row0 + 2 * cnt;
    for (int32_t k = 0; k < 2 * cnt; ++k) row0[k] = 0.0, row1[k] = 0.0;
    const double nu = m.nu, h = m.h;
    const int32_t q1 = m.inc_off[g + 1];
    for (int32_t q = m.inc_off[g]; q < q1; ++q) {
        const uint32_t w = m.inc[q];
        const int64_t e = w / 3u;
        const int a = (int)(w - 3u * (uint32_t)e);
        const int32_t n0 = m.conn[3 * e], n1 = m.conn[3 * e + 1], n2 = m.conn[3 * e + 2];
        const double2 x0 = m.xy[n0], x1 = m.xy[n1], x2 = m.xy[n2], u0 = u[n0], u1 = u[n1], u2 = u[n2];
        const double2 db = make_double2(x1.x - x0.x, x1.y - x0.y), dc = make_double2(x2.x - x0.x, x2.y - x0.y);
        TlNeo neo;
        const TlStrain s = tl_strain<LAW>(db, make_double2(u1.x - u0.x, u1.y - u0.y), dc, make_double2(u2.x - u0.x, u2.y - u0.y), nu, h, inverted, &neo);
        const double r = ring_rcp<double>(s.twoA);
        const double2 g0 = make_double2((db.y - dc.y) * r, (dc.x - db.x) * r), g1 = make_double2(dc.y * r, -(dc.x * r)),
                      g2 = make_double2(-(db.y * r), db.x * r);
        const double F11 = 1.0 + s.H11, F12 = s.H12, F21 = s.H21, F22 = 1.0 + s.H22;
        const double wv = s.twoA * m.c0; // V c
        const double2 gk = a == 0 ? g0 : (a == 1 ? g1 : g2);
        if constexpr (LAW == kLawNeoHooke) {
            // h_k = F^-T g_k = (F22 g.x - F21 g.y, F11 g.y - F12 g.x) / det F; the row's corner carries mu C33 too
            const double ri = 1.0 / fma(F11, F22, -(F12 * F21));
            const double c33 = 1.0 + neo.d;
            const double k2 = 2.0 * (nu / fma(2.0, c33, nu)); // 2 kappa (nu holds Lambda / mu)
            const double wc = c33 * ri;
            const double hkx = wc * fma(F22, gk.x, -(F21 * gk.y)), hky = wc * fma(F11, gk.y, -(F12 * gk.x));
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const double2 gl = l == 0 ? g0 : (l == 1 ? g1 : g2);
                const int32_t j = l == 0 ? n0 : (l == 1 ? n1 : n2);
                const double hlx = ri * fma(F22, gl.x, -(F21 * gl.y)), hly = ri * fma(F11, gl.y, -(F12 * gl.x));
                const double gg = fma(gk.x, gl.x, gk.y * gl.y);
                const double k00 = wv * (fma(k2, hkx * hlx, hlx * hkx) + gg);
                const double k01 = wv * fma(k2, hkx * hly, hlx * hky);
                const double k10 = wv * fma(k2, hky * hlx, hly * hkx);
                const double k11 = wv * (fma(k2, hky * hly, hly * hky) + gg);
                for (int32_t k = 0; k < cnt; ++k)
                    if (pat.bcol[p + k] == j) {
                        row0[2 * k] = row0[2 * k] + k00;
                        row0[2 * k + 1] = row0[2 * k + 1] + k01;
                        row1[2 * k] = row1[2 * k] + k10;
                        row1[2 * k + 1] = row1[2 * k + 1] + k11;
                        break;
                    }
            }
            continue;
        }
        // (D / c) B_k, column d: (p0 + nu p1, p1 + nu p0, h p2) of p = (F_d1 gk.x, F_d2 gk.y, F_d1 gk.y + F_d2 gk.x)
        const double pa0 = F11 * gk.x, pa1 = F12 * gk.y, pa2 = fma(F11, gk.y, F12 * gk.x);
        const double pb0 = F21 * gk.x, pb1 = F22 * gk.y, pb2 = fma(F21, gk.y, F22 * gk.x);
        const double da0 = fma(nu, pa1, pa0), da1 = fma(nu, pa0, pa1), da2 = h * pa2;
        const double db0 = fma(nu, pb1, pb0), db1 = fma(nu, pb0, pb1), db2 = h * pb2;
        // (S / c) g_k
        const double tx = fma(s.sx, gk.x, s.tq * gk.y), ty = fma(s.tq, gk.x, s.sy * gk.y);
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const double2 gl = l == 0 ? g0 : (l == 1 ? g1 : g2);
            const int32_t j = l == 0 ? n0 : (l == 1 ? n1 : n2);
            const double qa0 = F11 * gl.x, qa1 = F12 * gl.y, qa2 = fma(F11, gl.y, F12 * gl.x);
            const double qb0 = F21 * gl.x, qb1 = F22 * gl.y, qb2 = fma(F21, gl.y, F22 * gl.x);
            const double geo = fma(tx, gl.x, ty * gl.y);
            const double k00 = wv * (fma(da0, qa0, fma(da1, qa1, da2 * qa2)) + geo);
            const double k01 = wv * fma(da0, qb0, fma(da1, qb1, da2 * qb2));
            const double k10 = wv * fma(db0, qa0, fma(db1, qa1, db2 * qa2));
            const double k11 = wv * (fma(db0, qb0, fma(db1, qb1, db2 * qb2)) + geo);
            for (int32_t k = 0; k < cnt; ++k) // (the column is one of the row's: K couples the same pairs)
                if (pat.bcol[p + k] == j) {
                    row0[2 * k] = row0[2 * k] + k00;
                    row0[2 * k + 1] = row0[2 * k + 1] + k01;
                    row1[2 * k] = row1[2 * k] + k10;
                    row1[2 * k + 1] = row1[2 * k + 1] + k11;
                    break;
                }
        }
    }
    if (EFFECTIVE)
        for (int32_t k = 0; k < cnt; ++k) { // (k_tr_effective's expression, both scalar rows of the block row)
            const double mm = c_M * mval[p + k];
            const double a0 = c_K * row0[2 * k], a1 = c_K * row0[2 * k + 1], b0 = c_K * row1[2 * k], b1 = c_K * row1[2 * k + 1];
            row0[2 * k] = a0 + mm;
            row0[2 * k + 1] = a1;
            row1[2 * k] = b0;
            row1[2 * k + 1] = b1 + mm;
        }
}

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
