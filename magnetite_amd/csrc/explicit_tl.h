// Internal: launch wrappers of explicit_tl.hip (explicit dynamics with large rotations, mag_run_explicit with kinematics =
// MAG_KIN_TOTAL_LAGRANGIAN, and mag_internal_force): the total-Lagrangian internal force of a St. Venant-Kirchhoff plane-stress
// material in the reference configuration, as a fused central-difference step on the tile-local ring tables and as a kernel in
// caller numbering over the incidence lists.
//
// The method.  The step is explicit.h's with K (ut + eta vt) replaced by f_int(ut) (eta must be 0: initial-stiffness damping is
// not objective).  For a triangle (a, b, c) with the reference edges db = X_b - X_a, dc = X_c - X_a and the relative displacements
// ub = u_b - u_a, uc = u_c - u_a:
//   2A = db x dc
//   H = grad u:   H11 = (dc.y ub.x - db.y uc.x) / 2A    H12 = (db.x uc.x - dc.x ub.x) / 2A
//                 H21 = (dc.y ub.y - db.y uc.y) / 2A    H22 = (db.x uc.y - dc.x ub.y) / 2A
//   F = I + H
//   Green-Lagrange strain:   Exx = H11 + (H11^2 + H21^2) / 2,   Eyy = H22 + (H12^2 + H22^2) / 2,
//                            Gxy = H12 + H21 + H11 H12 + H21 H22
//   second Piola-Kirchhoff stress, c = E / (1 - nu^2):   Sxx = c (Exx + nu Eyy),   Syy = c (Eyy + nu Exx),   Sxy = c (1 - nu) / 2 Gxy
//     (the constants c0 = c t / 2, nu, h = (1 - nu) / 2 that fan_force takes)
//   first Piola-Kirchhoff stress P = F S;   the force on corner a is (t / 2) P (db.y - dc.y, dc.x - db.x)^T
//   the element's strain energy is A t (Sxx Exx + Syy Eyy + Sxy Gxy) / 2
// Without the quadratic terms of E and with F = I this is fan_force: the linearisation at u = 0 is the project's K, and a rigid
// motion u = (R - I)(X - X_c) + d gives zero force.
//   step:       a' = (amplitude[n+1] f - alpha m vt - f_int(ut))_F / ((1 + dt alpha / 2) m),   a'_P = 0
//   reactions:  f_int(u) on P (a = v = 0 there), amplitude[n] f on F
//   energies:   T = 1/2 v.mv,   W = sum over the elements of W_e,   P = amplitude[n] f.u_F
// An element with det F <= 0 is inverted: the kernels raise an integer flag (one atomicOr behind the test) and go on.
//
// The material law (mag_set_material_law) is a compile-time parameter LAW of the device functions and of the kernels that call
// them; the host picks the instantiation from TlMesh::law / ExplicitTlParams::law.  kLawSvk is the text above, expression for
// expression.  kLawNeoHooke is the compressible neo-Hooke material with the plane-stress condition enforced per triangle:
//   W = mu/2 (tr C + C33 - 3) - mu ln J + Lambda/2 (ln J)^2,   C = F^T F,  j2 = det C,  J^2 = j2 C33,
//   mu = E / (2 (1 + nu)),  Lambda = E nu / ((1 + nu)(1 - 2 nu))
//   j2 - 1 = j2m1 = 2 (Exx + Eyy) + 4 Exx Eyy - Gxy^2          (from the strains: no cancellation against 1)
//   S33 = 0:  g(d) = d + (Lambda / mu) / 2 (log1p(j2m1) + log1p(d)) = 0  for  d = C33 - 1   (neo_thickness below)
//   S = mu (I - C33 C^-1), written over the common denominator j2 so that small strains do not cancel against 1:
//     Sxx = mu (2 Exx + (4 Exx Eyy - Gxy^2) - d (1 + 2 Eyy)) / j2,   Syy = mu (2 Eyy + (4 Exx Eyy - Gxy^2) - d (1 + 2 Exx)) / j2,
//     Sxy = mu (1 + d) Gxy / j2                                  (C^-1's off-diagonal is -Gxy / j2)
//   P = F S and the force on a corner as above; in closed form it is V mu (F g_k - C33 F^-T g_k)
//   W_e = A t mu ((2 (Exx + Eyy) + d) / 2 - l + (Lambda / mu) l^2 / 2),   l = ln J = (log1p(j2m1) + log1p(d)) / 2
// Under kLawNeoHooke the three constants carry  c0 = mu t / 2,  nu = Lambda / mu = 2 nu / (1 - 2 nu),  h: not read,  and
// s = S / mu.  u = 0 gives d = 0 and S = 0 exactly; nu = 0 gives d = 0 always.  Nothing is special-cased for an inverted element:
// det F < 0 gives finite numbers from j2 = (det F)^2, det F = 0 gives non-finite ones, which the passes' finite checks catch.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "cg_device.h"
#include "explicit.h"

namespace magk {

// the material laws: enum mag_material_law's values
constexpr int kLawSvk = 0, kLawNeoHooke = 1;

// d = C33 - 1 of the plane-stress condition g(d) = d + lr / 2 (L + log1p(d)) = 0, L = log1p(j2m1), lr = Lambda / mu.  For lr >= 0
// g is increasing and concave, and Newton's method from d0 = min(0, -j2m1 / j2) -- g(0) = lr L / 2 <= 0 where j2 <= 1, and
// g(1 / j2 - 1) = 1 / j2 - 1 <= 0 where j2 >= 1 -- rises monotonically to the root: iterate while the iterate still increases.
// For lr < 0 (nu < 0) g is convex and the iterates, past the root after the first step, fall to it: then while they still fall.
// A counted loop (at most 15 iterations over j2 = 1e-6 .. 1e6 and nu up to 0.499; the cap is never reached); a non-finite j2 ends
// it at once, every comparison being false.
constexpr int kNeoSolveCap = 40;
__device__ inline double neo_thickness(double j2m1, double L, double lr)
{
    const double hl = 0.5 * lr;
    double d = fmin(0.0, -j2m1 / (1.0 + j2m1));
    bool fell = false;
    for (int k = 0; k < kNeoSolveCap; ++k) {
        const double gv = fma(hl, L + log1p(d), d), gp = 1.0 + hl / (1.0 + d);
        const double dn = d - gv / gp;
        if (dn > d && !fell) {
            d = dn;
        } else if (lr < 0.0 && dn < d) {
            d = dn;
            fell = true;
        } else {
            break;
        }
    }
    return d;
}

// Green-Lagrange strain and the scaled stress of one triangle given relative to its corner a; s = S / c
struct TlStrain {
    double twoA, H11, H12, H21, H22, Exx, Eyy, Gxy, sx, sy, tq;
};
// kLawNeoHooke: s = S / mu, and what the energy and the tangent need of the local solve
struct TlNeo {
    double d, lj; // C33 - 1, ln J
};

// (every multiply-add is written as the fma() it is: the unit is compiled -ffp-contract=off)
template <int LAW>
__device__ inline TlStrain tl_strain(const double2 db, const double2 ub, const double2 dc, const double2 uc, double nu, double h, int32_t *inverted,
                                     TlNeo *neo = nullptr)
{
    TlStrain s;
    s.twoA = fma(db.x, dc.y, -(dc.x * db.y));
    const double r = ring_rcp<double>(s.twoA);
    s.H11 = fma(dc.y, ub.x, -(db.y * uc.x)) * r;
    s.H12 = fma(db.x, uc.x, -(dc.x * ub.x)) * r;
    s.H21 = fma(dc.y, ub.y, -(db.y * uc.y)) * r;
    s.H22 = fma(db.x, uc.y, -(dc.x * ub.y)) * r;
    s.Exx = fma(0.5, fma(s.H11, s.H11, s.H21 * s.H21), s.H11);
    s.Eyy = fma(0.5, fma(s.H12, s.H12, s.H22 * s.H22), s.H22);
    s.Gxy = (s.H12 + s.H21) + fma(s.H11, s.H12, s.H21 * s.H22);
    if constexpr (LAW == kLawSvk) {
        s.sx = fma(nu, s.Eyy, s.Exx);
        s.sy = fma(nu, s.Exx, s.Eyy);
        s.tq = h * s.Gxy;
    } else { // (nu holds Lambda / mu)
        const double q = fma(4.0 * s.Exx, s.Eyy, -(s.Gxy * s.Gxy));
        const double j2m1 = 2.0 * (s.Exx + s.Eyy) + q;
        const double L = log1p(j2m1);
        const double d = neo_thickness(j2m1, L, nu);
        const double rj = 1.0 / (1.0 + j2m1);
        s.sx = (fma(2.0, s.Exx, q) - d * fma(2.0, s.Eyy, 1.0)) * rj;
        s.sy = (fma(2.0, s.Eyy, q) - d * fma(2.0, s.Exx, 1.0)) * rj;
        s.tq = ((1.0 + d) * s.Gxy) * rj;
        if (neo) neo->d = d, neo->lj = 0.5 * (L + log1p(d));
    }
    const double det = fma(1.0 + s.H11, 1.0 + s.H22, -(s.H12 * s.H21));
    if (det <= 0.0) atomicOr(inverted, 1);
    return s;
}

// fan_force with the total-Lagrangian internal force: adds the force of the triangle (a, b, c) on corner a to (fx, fy)
template <int LAW>
__device__ inline void fan_force_tl(const double2 db, const double2 ub, const double2 dc, const double2 uc, double c0, double nu, double h,
                                    double &fx, double &fy, int32_t *inverted)
{
    const TlStrain s = tl_strain<LAW>(db, ub, dc, uc, nu, h, inverted);
    const double ba = db.y - dc.y, ga = dc.x - db.x;
    const double qx = fma(ba, s.sx, ga * s.tq), qy = fma(ga, s.sy, ba * s.tq); // (S / c) (ba, ga)^T
    const double px = qx + fma(s.H11, qx, s.H12 * qy), py = qy + fma(s.H21, qx, s.H22 * qy); // F times it
    fx = fma(c0, px, fx);
    fy = fma(c0, py, fy);
}

// W_e = A t S:E / 2 = (2A) c0 (sx Exx + sy Eyy + tq Gxy) / 2
__device__ inline double tl_energy(const TlStrain &s, double c0)
{
    return (0.5 * s.twoA) * (c0 * fma(s.sx, s.Exx, fma(s.sy, s.Eyy, s.tq * s.Gxy)));
}
// kLawNeoHooke: W_e = A t mu ((2 (Exx + Eyy) + d) / 2 - l + lr l^2 / 2) = (2A) c0 (...)
__device__ inline double neo_energy(const TlStrain &s, const TlNeo &n, double c0, double lr)
{
    const double w = fma(0.5, fma(2.0, s.Exx + s.Eyy, n.d), -n.lj);
    return s.twoA * (c0 * fma(0.5 * lr, n.lj * n.lj, w));
}

struct ExplicitTlParams {
    StepFrame f;
    const double2 *xyP, *halo_xy;
    const int32_t *tile_deg; // ring words per row of the tile
    const int64_t *tile_off;
    const uint32_t *ell16; // the ring table (symbolic.hip, k_ring16)
    const int32_t *tile_hoff;
    double c0, nu, h;
    int32_t *inverted;
    int32_t law; // kLawSvk | kLawNeoHooke: which instantiation the host launches (c0, nu, h are that law's)
};

// workgroups of a step (step_grid) of the law's instantiation
int explicit_tl_grid(int32_t B, int32_t cap, int32_t tiles, int32_t law);
// one time step, one launch: reads P.f.in, writes P.f.out.  The order of a node's sum is its ring's (a function of the mesh and the
// tile size): the same bits for every grid, not across tile sizes
void explicit_tl_step(const ExplicitTlParams &P, int32_t B, int32_t grid, hipStream_t s);

// the mesh in caller numbering: the incidence lists by Hilbert position (mass_pattern's), the material
struct TlMesh {
    int64_t N, E;
    const uint32_t *perm;
    const int32_t *inc_off;
    const uint32_t *inc;
    const int32_t *conn;
    const double2 *xy;
    double c0, nu, h;
    int32_t law; // as ExplicitTlParams's
};

// the strain energy of element e, from its first corner (explicit_tl.hip, transient_tl.hip)
template <int LAW>
__device__ inline double tl_element_energy(const TlMesh &m, const double2 *u, int64_t e, int32_t *inverted)
{
    const int64_t a = m.conn[3 * e], b = m.conn[3 * e + 1], c = m.conn[3 * e + 2];
    const double2 ca = m.xy[a], cb = m.xy[b], cc = m.xy[c], ua = u[a], pb = u[b], pc = u[c];
    TlNeo neo;
    const TlStrain s = tl_strain<LAW>(make_double2(cb.x - ca.x, cb.y - ca.y), make_double2(pb.x - ua.x, pb.y - ua.y),
                                      make_double2(cc.x - ca.x, cc.y - ca.y), make_double2(pc.x - ua.x, pc.y - ua.y), m.nu, m.h, inverted, &neo);
    if constexpr (LAW == kLawSvk)
        return tl_energy(s, m.c0);
    else
        return neo_energy(s, neo, m.c0, m.nu);
}

// f[2N] = f_int(u), one lane per node, the triangles in the order of its incidence list; *inverted |= 1 for det F <= 0.
// energy != nullptr: also *energy = W(u), the elements' energies by a two-stage sum of a fixed shape (partials: scratch
// [kSensBlocks]).  One launch, or three
void tl_force(const TlMesh &m, const double *u, double *f, int32_t *inverted, double *partials, double *energy, hipStream_t s);

// the unfused step's acceleration: a = (amplitude[amp_at] f - (fint + m (alpha vt))) / (c m) on F, 0 on P (m the diagonal of mval)
void tl_divide(const Pattern &pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude, int64_t amp_at,
               const double *fint, const double *vt, double alpha, double c, double *a, hipStream_t s);
// the reactions: out = fint on P, amplitude[amp_at] f on F
void tl_reactions(const uint8_t *known, const double *f, const double *amplitude, int64_t amp_at, const double *fint, int64_t n2, double *out,
                  hipStream_t s);
// an energy row: out[0] = 1/2 v.mv, out[1] = W(u), out[2] = amplitude[amp_at] f.u_F; partials: scratch [kSensBlocks][3].
// Two launches; *inverted as tl_force
void tl_energies(const TlMesh &m, const Pattern &pat, const double *mval, const uint8_t *known, const double *u, const double *v, const double *f,
                 const double *amplitude, int64_t amp_at, int32_t *inverted, double *partials, double *out, hipStream_t s);

// the second stage of an energy row: out[0] = 1/2 partials' T, out[1] = their W, out[2] = amplitude[amp_at] times their f.u;
// partials: [kSensBlocks][3] (tl_energies', tl_dynamic_energies')
void tl_row_sum(const double *partials, const double *amplitude, int64_t amp_at, double *out, hipStream_t s);

} // namespace magk
