// Internal: launch wrapper of sens.hip (energy and design sensitivities of solved members, mag_run_sensitivities).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace magk {

constexpr int kSensBlocks = 256; // workgroups per member of the scalars' first stage: a fixed shape, whatever the mesh

// The head of every pass's batch (SensBatch, AdjointBatch, ObjectiveBatch): `count` solved members of one launch, grid.y = the
// member.  Every pointer of a batch is the FIRST member's; a stride of 0: every member reads the same array (the uploaded
// coordinates, the uploaded values).  member_of (member_pass.h) unpacks it on the device.
struct MemberBatch {
    int32_t count;
    int32_t pad;
    const double *mat;  // E, nu, thickness
    int64_t mat_stride; // doubles: 3 (a material per member) or 0
    const double *xy;   // caller-order coordinates
    int64_t xy_stride;  // doubles: 2N or 0
    const double *u;    // [count][2N] solved displacements, caller numbering
    const double *scale; // the element stiffness field (mag_set_element_scale): E values every member shares, or null -- then no
                         // term is multiplied by anything
};

struct SensBatch : MemberBatch {
    const double *f_out;  // [count][2N] forces with the reactions
    const double *u_in;   // prescribed values
    const double *f_in;
    int64_t loads_stride; // doubles: 2N or 0
    double *energy;       // out [count][E]
    double *dxy;          // out [count][2N]
    double *scalars;      // out [count][8]
    double *nuterm;       // scratch [count][E]: d(energy[e]) / d(nu)
    double *partials;     // scratch [count][kSensBlocks][4]
};

// The uploaded mesh and the tables of its ordering phase (all of the whole mesh, one rank).  tab: the tile-local corner table
// (fill_ell16's plain form: lb | lc << 16 per incident triangle, [tile_off[t] + k * B + l]), or null where the tile image of
// cap nodes does not fit the LDS (cap > kMaxLdsNodes): the node kernel then gathers from memory over inc_off / inc.
struct SensMesh {
    int64_t N, E;
    const int32_t *conn;
    const uint8_t *u_known;
    const uint32_t *perm;     // Hilbert position -> caller id
    const int32_t *inc_off;   // per Hilbert position
    const uint32_t *inc;      // 3e + corner, ascending per node
    int32_t B, T, cap;        // tile size, tiles, nodes of the largest tile image (owned + halo)
    const int32_t *halo_g;    // Hilbert positions of the tiles' halo nodes
    const int32_t *tile_hoff; // [T + 1] into halo_g
    const int32_t *tile_deg;  // [T] longest incidence list of the tile
    const int64_t *tile_off;  // [T + 1] into tab
    const uint32_t *tab;
};

// element energies, node gradients (per tile of the Hilbert order, sums in the order of the incidence lists) and the scalars of
// every member of sb: four launches
void sensitivities(const SensMesh &m, const SensBatch &sb, hipStream_t s);

} // namespace magk
