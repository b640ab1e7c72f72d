// Internal: launch wrappers of refine.hip (longest-edge refinement with conformity closure of the uploaded mesh, mag_run_refine).
// The host driver (api.hip) owns every buffer and runs the device-wide sorts and scans between the stages.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace magk {

constexpr int kRefineSweepBatch = 8; // closure sweeps per read-back of their "changed" words

// words of RefineTables::counters
enum RefineCounter {
    RF_MARKED = 0, // elements marked before the closure
    RF_SPLIT2 = 1, // elements split in two, three, four
    RF_SPLIT3 = 2,
    RF_SPLIT4 = 3,
    RF_NEW_NODES = 4, // marked edges
    RF_NEW_ELEMS = 5, // E'
    RF_CHANGED = 8,   // kRefineSweepBatch words: sweep j of the batch marked an edge
    RF_COUNTERS = 16
};

// The uploaded mesh and the tables of one refinement.  n3 = 3E.
struct RefineTables {
    int64_t N, E;
    const double *xy;       // [2N]
    const int32_t *conn;    // [3E]
    const uint8_t *u_known; // [2N]
    const double *u_in, *f_in;
    uint64_t *key0, *key1;  // [3E] edge keys lo << 32 | hi by slot 3e + k, then sorted; the top-fraction keys by element
    uint32_t *val0, *val1;  // [3E] their slots / elements
    int32_t *head, *hscan;  // [3E] run heads of the sorted keys, their exclusive scan
    int32_t *eid;           // [3E] edge id of slot 3e + k
    uint64_t *ekey;         // [3E] key of edge id
    uint32_t *flag;         // [3E + 1] one word per edge id: marked (the words past the last edge stay 0)
    int32_t *mid;           // [3E + 1] exclusive scan of flag, then the edge's new node or -1
    uint8_t *lng;           // [E] local index of the element's longest edge
    uint8_t *marks;         // [E]
    int32_t *cnt, *off;     // [E + 1] children per element (cnt[E] = 0), their exclusive scan (off[E] = E')
    uint32_t *counters;     // [RF_COUNTERS]
    uint64_t *check;        // [2]: bits of the largest valid indicator, the first entry that is not finite and >= 0 (or ~0)
};

// What mag_download_refine hands out, on the device.
struct RefinedMesh {
    double *xy;           // [2N']
    int32_t *conn;        // [3E']
    uint8_t *u_known;     // [2N']
    double *u_in, *f_in;  // [2N']
    int32_t *node_parents; // [N' - N][2]
    int32_t *elem_parent; // [E']
};

void refine_edge_keys(const RefineTables &t, hipStream_t s);  // key0, val0
void refine_heads(const RefineTables &t, hipStream_t s);      // head, from key1
void refine_edge_table(const RefineTables &t, hipStream_t s); // eid, ekey, lng, from the sorted keys and hscan
void refine_check_indicator(const RefineTables &t, const double *ind, hipStream_t s); // check
void refine_mark_max(const RefineTables &t, const double *ind, double threshold, hipStream_t s); // marks
void refine_top_keys(const RefineTables &t, const double *ind, hipStream_t s);    // key0, val0 [E]
void refine_mark_top(const RefineTables &t, int64_t k, hipStream_t s);            // marks, from val1 (marks zeroed before)
void refine_mark_edges(const RefineTables &t, int split, hipStream_t s);          // flag, counters[RF_MARKED]
void refine_sweeps(const RefineTables &t, int sweeps, hipStream_t s);             // <= kRefineSweepBatch closure sweeps
void refine_child_counts(const RefineTables &t, hipStream_t s);                   // cnt, counters[RF_SPLIT*]
void refine_sizes(const RefineTables &t, hipStream_t s);                          // counters[RF_NEW_NODES, RF_NEW_ELEMS]
void refine_emit(const RefineTables &t, const RefinedMesh &out, hipStream_t s);   // the new nodes, then the elements

} // namespace magk
