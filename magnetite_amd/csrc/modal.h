// Internal: launch wrappers of modal.hip (modal analysis, mag_run_modal: the mass operator, the Gram matrices of the
// Rayleigh-Ritz step, the rotation of the subspace, its start vectors, the orientation check, the modes' norms and signs).
// Vectors lie [count][2N] in the caller's numbering, as the member sets store theirs.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "sens.h"

namespace magk {

constexpr int kModalMaxQ = 32;  // vectors of the subspace at most
constexpr int kModalGramCols = 4; // columns j of one workgroup row of the Gram stage: 2 * kModalGramCols sums per thread

// `count` vectors on the uploaded mesh (MemberBatch with xy_stride = mat_stride = 0: one mesh, many vectors; u = the vectors x)
struct MassBatch : MemberBatch {
    double *y;       // out [count][2N]: M x
    double density;  // rho: m_e = rho * thickness * |A_e|
    int32_t lumped;  // != 0: m_e / 3 on each corner's diagonal
    int32_t masked;  // != 0: rows of prescribed DOFs are written as 0
};

// workgroup rows (grid.y) of the Gram stage for q vectors: q * ceil(q / kModalGramCols)
inline int32_t gram_rows(int32_t q) { return q * ((q + kModalGramCols - 1) / kModalGramCols); }

// y = M x for every vector of mb, per node over the node's incidence list in list order: per tile of the Hilbert order on an
// LDS image of 32 bytes per node, or gathered from memory where m.tab is null -- the same bits either way.  One launch.
void mass_apply(const SensMesh &m, const MassBatch &mb, hipStream_t s);

// X = 0 on prescribed DOFs, for `count` vectors
void mask_vectors(const uint8_t *u_known, int64_t N, int32_t count, double *X, hipStream_t s);

// A = Z^T Y and B = Z^T W (q x q each, row major, A then B in `out`; not symmetrised) for Z, Y, W [q][2N]: the two-stage
// reduction of member_pass.h; partials: scratch [gram_rows(q)][kSensBlocks][2 * kModalGramCols].  Two launches.
void gram(const double *Z, const double *Y, const double *W, int64_t N, int32_t q, double *partials, double *out, hipStream_t s);

// X = Z Q and Ynew = W Q in one launch (qs: Q as [kModalMaxQ][kModalMaxQ] row major, column k = Ritz vector k, zero past q,
// then lambda[kModalMaxQ]); with R, also R_k = (Yold Q)_k - lambda_k Ynew_k for k < modes.  Ynew must not be Yold or W.
void rotate(const double *Z, const double *W, const double *Yold, const double *qs, int64_t N, int32_t q, int32_t modes, double *X,
            double *Ynew, double *R, hipStream_t s);

// out[2 k] = |R_k|^2, out[2 k + 1] = |Y_k|^2 for k < modes; partials: scratch [modes][kSensBlocks][2].  Two launches.
void residual_norms(const double *R, const double *Y, int64_t N, int32_t modes, double *partials, double *out, hipStream_t s);

// the q start vectors: DOF d of node i in vector j = a fixed integer hash of the bits of the node's coordinates and of 2 j + d,
// in [-1, 1), 0 on prescribed DOFs (tests/modal_ref.py hash_unit is its twin)
void start_vectors(const double *xy, const uint8_t *u_known, int64_t N, int32_t q, double *X, hipStream_t s);

// *bad = the first element whose signed area is not positive (all ones: none) -- an integer minimum, by offenders only
void orientation(const double *xy, const int32_t *conn, int64_t N, int64_t E, unsigned long long *bad, hipStream_t s);

// every one of the `modes` vectors of X gets the sign that makes its entry of largest magnitude positive (on a tie the first in
// caller order).  One workgroup per vector.
void fix_signs(double *X, int64_t N, int32_t modes, hipStream_t s);

} // namespace magk
