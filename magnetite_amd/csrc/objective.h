// Internal: launch wrappers of objective.hip (mag_run_objective: an objective J of solved members, dJ/du and J's explicit
// partials at fixed u, and the totals once the adjoint pass has run).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "sens.h"

namespace magk {

// The members of one launch (MemberBatch, sens.h) with the objective.
struct ObjectiveBatch : MemberBatch {
    int32_t kind;          // enum mag_objective_kind
    const double *w;       // weights: 2N per row (MAG_OBJ_DISP_LSQ), E per row or null = ones (MAG_OBJ_STRESS_PNORM)
    int64_t w_stride;      // doubles: the row's length (a row per member) or 0
    const double *target;  // MAG_OBJ_DISP_LSQ: 2N per row, or null = zeros
    int64_t target_stride; // doubles: 2N or 0
    double p, scale;       // MAG_OBJ_STRESS_PNORM
    double *g;             // out [count][2N] dJ/du
    double *pxy;           // out [count][2N] dJ/dxy at fixed u
    double *scalars;       // out [count][8]: J, the explicit dJ/dE, dJ/dnu, dJ/dt; 4..7 = 0 until objective_totals
    double *terms;         // scratch [count][n] the objective's summands: n = E (p-norm) or 2N (least squares)
    double *nuterm;        // scratch [count][E], p-norm: the summands of dS/dnu
    double *helem;         // scratch [count][E], p-norm: w_e (vm_e / scale)^(p - 2), what the node kernel scales a corner by
    double *partials;      // scratch [count][kSensBlocks][2]
    double *factor;        // scratch [count], p-norm: S^(1/p - 1) / (2 scale), 0 where S = 0
};

// J, g, pxy and the explicit scalars of every member of ob.  The p-norm: elements, the two-stage reduction (which leaves the
// member's factor on the device), then the nodes -- per tile of the Hilbert order on an LDS image of 32 bytes per node, or gathered
// from memory where m.tab is null; four launches.  Least squares: one launch per DOF, the reduction; pxy is zeroed.
void objective(const SensMesh &m, const ObjectiveBatch &ob, hipStream_t s);

// dxy[v] = pxy[v] + adj_dxy[v] (one add per entry) and scalars[v][4..6] = scalars[v][1..3] + adj_scalars[v][1..3],
// scalars[v][7] = 1, for `count` members: one launch.
void objective_totals(int64_t N, int32_t count, const double *pxy, const double *adj_dxy, const double *adj_scalars, double *dxy,
                      double *scalars, hipStream_t s);

} // namespace magk
