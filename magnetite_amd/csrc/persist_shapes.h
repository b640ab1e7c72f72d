// The instantiations of the on-chip CG kernel (persist_kernel.h, k_cg_persist): which exist, which object holds each, and which
// one a launch takes.  Stated here once; the objects generate their instantiations from these lists, persist_launch selects
// with persist_shape.  Plain C++ with no HIP type in it: tests/cpp/persist_shapes.cpp compiles it with the host compiler alone.
#pragma once
#include <cstdint>

namespace magk {

// what a launch solves side by side (grid.y): one problem, load cases of one mesh (LC), design variants of it (LC and VAR)
enum PersistMembers { PERSIST_SINGLE, PERSIST_CASES, PERSIST_VARIANTS };

// k_cg_persist<B, mg, 512, ebm, one, nptx, members == PERSIST_VARIANTS, members != PERSIST_SINGLE>
struct PersistShape {
    int32_t B;  // nodes per tile
    bool mg;    // several GPUs: the exchange through the ranks' inboxes
    int ebm;    // 0 triangle walk, 1 edge blocks, 2 edge blocks with overflow records in LDS
    bool one;   // the whole mesh in one workgroup: no exchange through memory
    int nptx;   // node slots per lane: 1 to 3, or 0 for the general four
    PersistMembers members;
};

// One list per object, a row X(B, mg, ebm, one, nptx).  Every object is compiled with -ffp-contract=off; what differs is the
// instruction scheduler, a per-translation-unit option -- hence the objects.

// persist.o, iterative-ilp: the kernel has two waves per SIMD and is fp64-issue bound -- 11.7 us per iteration against 12.6 under
// the default scheduler (max-ilp 12.0, max-memory-clause 12.05).  The general four-slot kernels of both tile sizes, one GPU and
// several; the 512-node edge-block kernels with one to three node slots (0.45 us per iteration less than four slots of which
// some are dead), without an exchange where one workgroup holds the whole mesh, and across ranks.
#define MAG_PERSIST_ROWS_MAIN(X)                                                                                                  \
    X(256, true, 2, false, 0) X(512, true, 2, false, 0) X(256, true, 1, false, 0) X(512, true, 1, false, 0)                       \
    X(256, true, 0, false, 0) X(512, true, 0, false, 0)                                                                           \
    X(256, false, 2, false, 0) X(512, false, 2, false, 0) X(256, false, 1, false, 0)                                              \
    X(256, false, 0, false, 0) X(512, false, 0, false, 0)                                                                         \
    X(512, false, 1, false, 1) X(512, false, 1, false, 2) X(512, false, 1, false, 3)                                              \
    X(512, false, 2, false, 1) X(512, false, 2, false, 2) X(512, false, 2, false, 3)                                              \
    X(512, false, 1, true, 1) X(512, false, 1, true, 2) X(512, false, 1, true, 3)                                                 \
    X(512, false, 2, true, 1) X(512, false, 2, true, 2) X(512, false, 2, true, 3)                                                 \
    X(512, false, 1, true, 0) X(512, false, 2, true, 0)                                                                           \
    X(512, true, 1, false, 1) X(512, true, 1, false, 2) X(512, true, 1, false, 3)                                                 \
    X(512, true, 2, false, 1) X(512, true, 2, false, 2) X(512, true, 2, false, 3)

// persist_k4.o, max-ilp: the four-slot edge-block kernel of ONE GPU -- the kernel of BASELINE config 3 -- measured 5.43 against
// 5.52 us per iteration at 1M triangles under it in one session, while every other instantiation is FASTER under iterative-ilp
// (one / two / three node slots 3.48 / 4.08 / 4.65 against 3.53 / 4.16 / 4.83; the overflow instantiation indifferent).  The
// stamped build has no such object: there the row is persist_stamps.o's.
#define MAG_PERSIST_ROWS_K4(X) X(512, false, 1, false, 0)

// persist_cases.o, iterative-ilp (persist.o's flags): the load-case kernels, in an object of their own so that persist.o and
// persist_k4.o keep their code objects.  One row per shape the single-problem path runs for a 512-node-tile mesh of which at
// least two cases fit the chip -- the SAME shape, so that a case gets the bits of a launch of its own.
#define MAG_PERSIST_ROWS_CASES(X)                                                                                                 \
    X(512, false, 0, false, 0)                                                                                                    \
    X(512, false, 1, false, 1) X(512, false, 1, true, 1) X(512, false, 1, true, 2) X(512, false, 1, true, 3)                      \
    X(512, false, 1, true, 0)                                                                                                     \
    X(512, false, 2, false, 1) X(512, false, 2, true, 1) X(512, false, 2, true, 2) X(512, false, 2, true, 3)                      \
    X(512, false, 2, true, 0)

// persist_variants.o, iterative-ilp (persist.o's flags): the design-variant kernels -- the load-case shapes, one for one
#define MAG_PERSIST_ROWS_VARIANTS(X) MAG_PERSIST_ROWS_CASES(X)

#define MAG_PERSIST_MEMBERS_MAIN PERSIST_SINGLE
#define MAG_PERSIST_MEMBERS_K4 PERSIST_SINGLE
#define MAG_PERSIST_MEMBERS_CASES PERSIST_CASES
#define MAG_PERSIST_MEMBERS_VARIANTS PERSIST_VARIANTS

// The shape of a launch of `grid` workgroups with `tiles_per_wg` tiles each; false: there is no such instantiation.
//   * The triangle walk takes the general four-slot kernel whatever the grid: it keeps halo COPIES of sibling nodes in tiles whose
//     rows do not fit its registers and advances them with q fetched from the granules, so it goes through the exchange even alone
//     on the grid.
//   * Edge blocks on 512-node tiles: as many node slots as the workgroup has tiles when those are fewer than four (meshes below
//     769 tiles, 393k nodes; a 1M-triangle mesh over four or eight GPUs is one tile per workgroup), and on one GPU the kernel
//     without an exchange when the grid is one workgroup -- its tiles read every sibling's node through LDS.
//   * Load cases and variants: one GPU, 512-node tiles, and of the shapes above those of a mesh of which two fit the chip -- one
//     workgroup of one to four tiles, or one tile per workgroup.
inline bool persist_shape(int32_t B, int32_t nranks, int32_t grid, int32_t tiles_per_wg, int eb_mode, PersistMembers m,
                          PersistShape &out)
{
    if ((B != 256 && B != 512) || nranks < 1 || grid < 1 || tiles_per_wg < 1 || eb_mode < 0 || eb_mode > 2) return false;
    const bool set = m != PERSIST_SINGLE;
    if (set && (nranks != 1 || B != 512 || tiles_per_wg > 4)) return false;
    out = PersistShape{B, nranks > 1, eb_mode, false, 0, m};
    if (eb_mode == 0) return true;
    if (B == 512) {
        out.one = nranks == 1 && grid == 1;
        out.nptx = tiles_per_wg <= 3 ? tiles_per_wg : 0;
    }
    return !set || out.one || tiles_per_wg == 1;
}

} // namespace magk
