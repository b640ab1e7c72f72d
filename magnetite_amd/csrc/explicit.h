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

struct ExplicitParams {
    int64_t N, total;
    int32_t T, cap;
    const uint8_t *maskP; // bit 0 / 1: prescribed ux / uy
    const FieldTileMeta *meta;
    const uint16_t *slot;
    const double2 *fval; // the unmasked block rows: plane 0 at fval, plane 1 at fval + total
    const int32_t *halo_g;
    const ExRec *in;
    ExRec *out;
    const double2 *uinP, *fP; // u_in and f_in, Hilbert order
    const double *massP;      // the node masses, Hilbert order
    const double *amplitude;
    int64_t amp_at; // the step's load is amplitude[amp_at] f
    double dt, alpha, eta;
};

// workgroups of a step: all co-resident, capped by MAG_TUNE_GRID and by the tile count (as field_cg_grid)
int explicit_grid(int32_t B, int32_t cap, int32_t tiles);
// one time step, one launch: reads P.in, writes P.out.  The row order (the diagonal, then ascending Hilbert index) is the
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
