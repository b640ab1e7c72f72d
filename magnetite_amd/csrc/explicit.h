// Internal: launch wrappers of explicit.hip (explicit dynamics, mag_run_explicit: central differences on the lumped mass -- a
// whole time step in one launch over the tile-local block rows of the assembled K, the stable-step bound, the moves between the
// caller's numbering and the Hilbert-ordered state records, the finite check).
//
// The method (Newmark with beta = 0, gamma = 1/2, the lumped mass m, C = alpha M + eta K with the eta term at the half-step
// velocity).  F: DOFs with u_known == 0, P: the supports, held at the uploaded u_in (v_P = a_P = 0).
//   step:   ut = u + dt v + dt^2/2 a,   vt = v + dt/2 a            (on P: ut = u_in, vt = 0)
//           a' = (amplitude[n+1] f - alpha m vt - K (ut + eta vt))_F / ((1 + dt alpha / 2) m),   a'_P = 0
//           u' = ut,   v' = vt + dt/2 a'
//   start:  the step with dt = 0 and amplitude[0]: a_0 = (amplitude[0] f - alpha m v_0 - K (u_0 + eta v_0))_F / m
// Prescribed displacements enter through K ut: the gathered block rows are NOT masked (field_gather under a zero mask).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "transient.h"

namespace magk {

// the state of one node, Hilbert order: 48 bytes
struct ExRec {
    double2 u, v, a;
};

// what the two step kernels (k_explicit_step, explicit_tl.hip's k_explicit_tl_step) share: the tiles, the records, the inputs in
// Hilbert order and the step
struct StepFrame {
    int64_t N;
    int32_t T, cap;
    const uint8_t *maskP; // bit 0 / 1: prescribed ux / uy
    const int32_t *halo_g;
    const ExRec *in;
    ExRec *out;
    const double2 *uinP, *fP; // u_in and f_in, Hilbert order
    const double *massP;      // the node masses, Hilbert order
    const double *amplitude;
    int64_t amp_at; // the step's load is amplitude[amp_at] f
    double dt, alpha;
};

// (Where the frame stands among a kernel's arguments decides how the compiler batches their scalar loads: here behind the
// kernel's own, in ExplicitTlParams in front of them, every argument arrives in one batch and the load of amplitude[amp_at], which
// depends on them, stays in flight until the corrector.  The other way round it is waited for in the prologue: 4 % of a step.)
struct ExplicitParams {
    int64_t total;
    const FieldTileMeta *meta;
    const uint16_t *slot;
    const double2 *fval; // the unmasked block rows: plane 0 at fval, plane 1 at fval + total
    double eta;
    StepFrame f;
};

// ---- the frame of a step, used by both kernels (both units are compiled -ffp-contract=off)
// the step's coefficients
struct StepCoef {
    double c_ua, c_va, c_den, amp;
};
__device__ __forceinline__ StepCoef step_coef(const StepFrame &F)
{
    StepCoef c;
    c.c_ua = F.dt * F.dt * 0.5;
    c.c_va = F.dt * 0.5;
    c.c_den = 1.0 + c.c_va * F.alpha;
    c.amp = F.amplitude[F.amp_at];
    return c;
}

// the predictors of one node; on P: ut = u_in, vt = 0
__device__ __forceinline__ void explicit_predict(const ExRec &r, const uint8_t m, const double2 uin, const double c_uv, const double c_ua,
                                                 const double c_va, double2 &ut, double2 &vt)
{
    ut.x = (m & 1) ? uin.x : (r.u.x + c_uv * r.v.x) + c_ua * r.a.x;
    ut.y = (m & 2) ? uin.y : (r.u.y + c_uv * r.v.y) + c_ua * r.a.y;
    vt.x = (m & 1) ? 0.0 : r.v.x + c_va * r.a.x;
    vt.y = (m & 2) ? 0.0 : r.v.y + c_va * r.a.y;
}

// the corrector of one node and its record: (kx, ky) is the internal force on it, K (ut + eta vt) or f_int(ut)
__device__ __forceinline__ void explicit_correct(const StepFrame &F, const StepCoef &c, const int64_t node, const uint8_t m, const double2 ut,
                                                 const double2 vt, const double2 fl, const double mass, const double kx, const double ky)
{
    const double den = c.c_den * mass;
    double2 an, vn;
    an.x = (m & 1) ? 0.0 : (c.amp * fl.x - (kx + mass * (F.alpha * vt.x))) / den;
    an.y = (m & 2) ? 0.0 : (c.amp * fl.y - (ky + mass * (F.alpha * vt.y))) / den;
    vn.x = vt.x + c.c_va * an.x;
    vn.y = vt.y + c.c_va * an.y;
    ExRec o;
    o.u = ut;
    o.v = vn;
    o.a = an;
    F.out[node] = o;
}

// a step kernel's workgroup size for tile size B, and its workgroups: all co-resident (the occupancy of `kernel` at `threads`
// and `lds` bytes), capped by MAG_TUNE_GRID and by the tile count (as field_cg_grid)
inline int step_threads(int32_t B) { return B == 256 || B == 1024 ? B : 512; }
int step_grid(const void *kernel, int threads, size_t lds, int32_t tiles);

// workgroups of a step of k_explicit_step (step_grid)
int explicit_grid(int32_t B, int32_t cap, int32_t tiles);
// one time step, one launch: reads P.f.in, writes P.f.out.  The row order (the diagonal, then ascending Hilbert index) is the
// table's and a function of the mesh alone: the same bits for every tile size and grid
void explicit_step(const ExplicitParams &P, int32_t B, int32_t grid, hipStream_t s);

// massP[g] = the diagonal entry of mval (mass_pattern, lumped) of node perm[g]; uinP, fP: u_in, f_in by Hilbert position
void explicit_inputs(const Pattern &pat, const uint32_t *perm, const double *mval, const double *u_in, const double *f_in, double *massP,
                     double2 *uinP, double2 *fP, hipStream_t s);
// rec[g] = (u, v, a)[perm[g]] and back: the caller-numbered state (2N each) and the records
void explicit_gather(const uint32_t *perm, int64_t N, const double *u, const double *v, const double *a, ExRec *rec, hipStream_t s);
void explicit_scatter(const uint32_t *perm, int64_t N, const ExRec *rec, double *u, double *v, double *a, hipStream_t s);

// out[0] = lambda_bound = max over free DOFs i of (sum over free j of |K_ij|) / m_i (Gershgorin on M_FF^-1 K_FF; 0 without a
// free DOF), out[1] = the smallest node mass.  partials: scratch [kSensBlocks][2].  Two launches, a fixed shape.
void explicit_bound(const Pattern &pat, const double *kval, const double *mval, const uint8_t *known, double *partials, double *out,
                    hipStream_t s);

// a = rhs / (c m) on F, 0 on P (the unfused step: m the diagonal of mval by caller DOF)
void explicit_divide(const Pattern &pat, const double *mval, const uint8_t *known, const double *rhs, double c, double *a, hipStream_t s);

// *flag |= 1 when an entry of u, v or a (2N each) is not finite; the caller zeroes the flag
void explicit_finite(const double *u, const double *v, const double *a, int64_t n2, int32_t *flag, hipStream_t s);

} // namespace magk
