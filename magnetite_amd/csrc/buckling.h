// Internal: launch wrappers of buckling.hip (linearised buckling, mag_run_buckling: the geometric stiffness of a solved member
// as an operator on many vectors and in K's block-CSR pattern).  Vectors lie [count][2N] in the caller's numbering.
//
// The classical linearised problem: (K_FF + lambda K_G,FF) phi_F = 0 with K the stiffness at the reference configuration and
// K_G the geometric stiffness of the LINEAR prestress sigma(u0) -- the initial-displacement terms of dK_T / dlambda are dropped.
// In the notation of member_pass.h (b, g the edge differences, A2 = 2A signed, p, q, r the cyclic sums of u0), cs = E / (1 - nu^2):
//   sigma_e = (sx, sy, txy) = cs / A2 (p + nu q, nu p + q, (1 - nu) / 2 r)                  (recover.hip's tensor, the same bits)
//   g_k = (b_k, g_k) / A2, the shape function gradients
//   K_G,e[k, l] = t A_e (g_k^T sigma_e g_l) I_2 = h_kl I_2,   h_kl = t / (2 A2) ((sx b_k + txy g_k) b_l + (txy b_k + sy g_k) g_l)
// The corners enter edges_of and cyclic_sums as differences to the triangle's first corner (buckling.hip says why).
// This is newton.h's (g_k^T S g_l) I term with S = sigma(u0) and F = I.  sum_l h_kl = 0: a rigid translation is in K_G's kernel.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "sens.h"
#include "transient.h"

namespace magk {

// `count` vectors on the uploaded mesh (MemberBatch with xy_stride = mat_stride = 0; u = the vectors x) under ONE prestress
struct GeomBatch : MemberBatch {
    const double *u0; // [2N] the displacements of the solved member: stride 0 across the vectors
    double *y;        // out [count][2N]: sign K_G x
    double sign;      // 1, or -1 (the iteration's Y = -K_G X: the negation is exact)
    int32_t masked;   // != 0: rows of prescribed DOFs are written as 0
    int32_t pad2;
};

// y = sign K_G(sigma(u0)) x for every vector of gb, per node over the node's incidence list in list order: per tile of the
// Hilbert order on an LDS image of 48 bytes per node (coordinates, u0, x), or gathered from memory where m.tab is null -- the
// same bits either way, for every grid and on every repeat.  No matrix is read.  One launch.
hipError_t geometric_apply(const SensMesh &m, const GeomBatch &gb, hipStream_t s);

// val[block (i, j)] = sum over the triangles that hold i and j, in the order of i's incidence list, of h_ij I_2, in kval's layout
// (4 doubles per block, the row's (k00, k01) pairs first, its (k10, k11) pairs behind them: mag_assemble_csr's values).  mat: E, nu,
// thickness on the device.  One lane per row node, no atomics.  One launch.
void geometric_values(const SensMesh &m, const Pattern &pat, const double *xy, const double *mat, const double *u0, double *val,
                      hipStream_t s);

} // namespace magk
