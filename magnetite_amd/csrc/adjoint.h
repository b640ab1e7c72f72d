// Internal: launch wrapper of adjoint.hip (the bilinear pass of mag_run_adjoint: -lambda^T (dK/dtheta) u of solved members).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "sens.h"

namespace magk {

// The members of one launch (MemberBatch, sens.h) with their adjoint solutions.
struct AdjointBatch : MemberBatch {
    const double *lam;   // [count][2N] the adjoint solutions (0 on the prescribed DOFs)
    const double *g;     // [count][2N] dJ/du as the caller gave it
    const double *f_adj; // [count][2N] the adjoint solves' forces: (K lambda) on the prescribed DOFs
    double *dloads;      // out [count][2N]
    double *delem;       // out [count][E]
    double *dxy;         // out [count][2N]
    double *scalars;     // out [count][8]
    double *nuterm;      // scratch [count][E]: lambda_e^T (dK_e / dnu) u_e
    double *partials;    // scratch [count][kSensBlocks][2]
};

// dloads, delem, dxy (per tile of the Hilbert order on an LDS image of 48 bytes per node, or gathered from memory where
// m.tab is null) and the scalars of every member of ab: five launches.  The error of raising the node kernel's dynamic LDS
// limit, if any; launch errors are the caller's to fetch.
hipError_t adjoint_bilinear(const SensMesh &m, const AdjointBatch &ab, hipStream_t s);

} // namespace magk
