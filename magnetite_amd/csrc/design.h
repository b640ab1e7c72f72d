// Internal: launch wrappers of design.hip -- the check of an element stiffness field (mag_set_element_scale) and the density
// design update (mag_design_init, mag_design_step): SIMP interpolation, the one-ring density filter and its transpose, the
// optimality-criteria update with the volume constraint.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "sens.h"

namespace magk {

// The doubles a design keeps on the device between the launches of a step (ds_small): the bisection's bracket, the target
// and the sums the info words are made of.  No value of it is read back before the step is complete.
enum DesignWord {
    DW_LO = 0, DW_HI, DW_TARGET, DW_V_LO0, DW_V_HI0, DW_MAX_BQ, DW_AREA, DW_PAD,
    DW_INFO, // eight info words: mag_get_design_info
    DW_COUNT = DW_INFO + 8
};
constexpr int kDesignBisections = 100;
constexpr size_t kDesignPartials = 4 * (size_t)kSensBlocks; // doubles: two sums and two maxima per workgroup of stage one

struct DesignParams {
    double scale_min, rho_min, move, volume_fraction;
    int32_t penal, filter_passes;
};

// first[0] = the smallest index i with x[i] not finite, <= 0 or > upper; unchanged (the caller presets INT32_MAX) when none
void first_out_of_range(const double *x, int64_t n, double upper, int32_t *first, hipStream_t s);

// area[e] = the signed area of element e, corners in conn order; first[0] as above for an area that is not finite or <= 0
void design_areas(const SensMesh &m, const double *xy, double *area, int32_t *first, hipStream_t s);
// node_area[i] = the sum of area[e] over the triangles of node i, in the order of its incidence list (caller numbering)
void design_node_areas(const SensMesh &m, const double *xy, const double *area, double *node_area, hipStream_t s);
// small[DW_AREA] = the sum of the areas, small[DW_TARGET] = volume_fraction times it
void design_total_area(const double *area, int64_t E, double volume_fraction, double *partials, double *small, hipStream_t s);

// y = F x: the area-weighted node average of the element values, then the mean of an element's three node values
void design_filter(const SensMesh &m, const double *xy, const double *area, const double *node_area, const double *x, double *node,
                   double *y, hipStream_t s);
// x = F^T y
void design_filter_t(const SensMesh &m, const double *xy, const double *area, const double *node_area, const double *y, double *node,
                     double *x, hipStream_t s);

// scale[e] = scale_min + (1 - scale_min) rhof[e]^penal, the power by repeated multiplication
void design_interpolate(const double *rhof, int64_t E, const DesignParams &p, double *scale, hipStream_t s);
// dJ/drhof[e] = dJ/ds[e] (1 - scale_min) penal rhof[e]^(penal - 1);  dJ_ds null: dJ/ds[e] = -2 energy[e] / scale[e]
void design_chain(const double *dJ_ds, const double *energy, const double *scale, const double *rhof, int64_t E, const DesignParams &p,
                  double *dJ_drhof, hipStream_t s);

// The optimality-criteria update: Bq, the bracket, V(lo0), V(hi0), kDesignBisections halvings and rho_new at the last midpoint,
// all on the device.  Fills small[DW_INFO + 0, 1, 2, 4].
void design_oc(const double *rho, const double *dJ_drho, const double *w, int64_t E, const DesignParams &p, double *bq, double *rho_new,
               double *partials, double *small, hipStream_t s);
// small[DW_INFO + 0] = sum of w rho / small[DW_AREA] (the volume fraction of a design that has not stepped yet)
void design_volume(const double *rho, const double *w, int64_t E, double *partials, double *small, hipStream_t s);
// small[DW_INFO + 3] = mean of 4 rhof (1 - rhof)
void design_greyness(const double *rhof, int64_t E, double *partials, double *small, hipStream_t s);

} // namespace magk
