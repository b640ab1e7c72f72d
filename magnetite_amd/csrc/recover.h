// Internal: launch wrapper of recover.hip (stress recovery of solved members, mag_run_stress: the stress tensor per element,
// the area-weighted nodal field, the ZZ error indicator and their scalars).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "sens.h"

namespace magk {

// The members of one launch (MemberBatch, sens.h) with the recovery's rows.
struct StressBatch : MemberBatch {
    double *elem;     // out [count][E][4]: sx, sy, txy, vm
    double *node;     // out [count][N][4]: the averaged tensor and its vm, caller numbering
    double *eta2;     // out [count][E]
    double *scalars;  // out [count][8]: eta^2, U^2, eta_rel, max vm of the elements, of the nodes; 5..7 = 0
    double *uterm;    // scratch [count][E]: |A_e| t sigma_e^T C sigma_e
    double *partials; // scratch [count][kSensBlocks][2] sums (eta2, uterm), then [count][kSensBlocks][2] maxima (elements, nodes)
};

// elem, node (per tile of the Hilbert order on an LDS image of 32 bytes per node, sums in the order of the incidence lists, or
// gathered from memory where m.tab is null), eta2 and the scalars of every member of sb: five launches
void stress_recovery(const SensMesh &m, const StressBatch &sb, hipStream_t s);

} // namespace magk
