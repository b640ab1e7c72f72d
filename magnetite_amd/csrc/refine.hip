// Longest-edge refinement with conformity closure (Rivara) of the uploaded mesh (mag_run_refine): streaming passes over the E
// elements or their 3E edge slots, in the caller's numbering.  The result is a pure function of the inputs -- the numbering of
// edges, new nodes and children is the header's, no pass depends on an order of arrival:
//   edge id     rank of (lo, hi) among the unique edges (sorted keys lo << 32 | hi, run heads, their scan: the host driver);
//   len2        dx * dx + dy * dy with (dx, dy) = xy[hi] - xy[lo]: both elements of an edge compute the same bits
//               (compiled -ffp-contract=off: two products, one addition);
//   longest     the local edge of largest len2, on a tie the smaller edge id: a total order on the edges;
//   closure     an element with a marked edge gets its longest edge marked, swept until nothing changes.  The marked set is the
//               least fixed point of a monotone rule on a finite set, so it does not depend on which of a sweep's own writes a
//               sweep sees; the NUMBER of sweeps would, so a sweep reads a copy of the flags made before it (Jacobi); flags are
//               one 32-bit word per edge, written with relaxed device-scope atomic stores;
//   new nodes   marked edge number r in edge-id order becomes node N + r, the midpoint 0.5 * (x[lo] + x[hi]);
//   children    of element e at off[e] .. off[e + 1], the element rotated so that its longest edge comes first.
// No floating-point sum and no floating-point atomic anywhere.
#include "refine.h"

namespace magk {

namespace {

constexpr int kBlock = 256;

inline dim3 blocks_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

__device__ inline void flag_set(uint32_t *f) { __hip_atomic_store(f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline double len2_of(const double2 *xy, int32_t a, int32_t b)
{
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const double2 l = xy[lo], h = xy[hi];
    const double dx = h.x - l.x, dy = h.y - l.y;
    return dx * dx + dy * dy;
}

} // namespace

// ---- edge keys: slot i = 3e + k holds (conn[3e + k], conn[3e + (k + 1) % 3]) as lo << 32 | hi
__global__ void __launch_bounds__(kBlock) k_rf_edge_keys(const int32_t *conn, int64_t n3, uint64_t *key, uint32_t *val)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n3) return;
    const int64_t e3 = i - i % 3;
    const uint32_t a = (uint32_t)conn[i], b = (uint32_t)conn[e3 + (i - e3 + 1) % 3];
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    key[i] = (uint64_t)lo << 32 | hi;
    val[i] = (uint32_t)i;
}

// ---- run heads of the sorted keys
__global__ void __launch_bounds__(kBlock) k_rf_heads(const uint64_t *key, int64_t n3, int32_t *head)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n3) return;
    head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// ---- edge table: the id of every slot's edge, the key of every edge
__global__ void __launch_bounds__(kBlock) k_rf_edge_table(const uint64_t *key, const uint32_t *val, const int32_t *head,
                                                          const int32_t *hscan, int64_t n3, int32_t *eid, uint64_t *ekey)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n3) return;
    const int32_t h = head[i], id = hscan[i] + h - 1;
    eid[val[i]] = id;
    if (h) ekey[id] = key[i];
}

// ---- longest edge of every element
__global__ void __launch_bounds__(kBlock) k_rf_longest(const double2 *xy, const int32_t *conn, const int32_t *eid, int64_t E,
                                                       uint8_t *lng)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const int32_t n[3] = {conn[3 * e], conn[3 * e + 1], conn[3 * e + 2]};
    const int32_t id[3] = {eid[3 * e], eid[3 * e + 1], eid[3 * e + 2]};
    const double l[3] = {len2_of(xy, n[0], n[1]), len2_of(xy, n[1], n[2]), len2_of(xy, n[2], n[0])};
    int L = 0;
    if (l[1] > l[L] || (l[1] == l[L] && id[1] < id[L])) L = 1;
    if (l[2] > l[L] || (l[2] == l[L] && id[2] < id[L])) L = 2;
    lng[e] = (uint8_t)L;
}

// ---- the indicator: every entry finite and >= 0; the largest, as the bits of a non-negative double (which order as the values
// do), and the first offender, each by one integer atomic per workgroup
__global__ void __launch_bounds__(kBlock) k_rf_check_indicator(const double *ind, int64_t E, uint64_t *check)
{
    __shared__ uint64_t s_max[kBlock / 64], s_bad[kBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t vmax = 0, bad = ~uint64_t(0);
    if (e < E) {
        const double v = ind[e];
        if (v >= 0.0 && v <= 1.7976931348623157e308)
            vmax = (uint64_t)__double_as_longlong(v + 0.0);
        else
            bad = (uint64_t)e;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t m = __shfl_down(vmax, off), b = __shfl_down(bad, off);
        vmax = m > vmax ? m : vmax;
        bad = b < bad ? b : bad;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        s_max[w] = vmax;
        s_bad[w] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / 64; ++k) {
            vmax = s_max[k] > vmax ? s_max[k] : vmax;
            bad = s_bad[k] < bad ? s_bad[k] : bad;
        }
        if (vmax) atomicMax((unsigned long long *)&check[0], (unsigned long long)vmax);
        if (bad != ~uint64_t(0)) atomicMin((unsigned long long *)&check[1], (unsigned long long)bad);
    }
}

// ---- MAG_REFINE_MAX_FRACTION: marked iff ind[e] >= threshold (theta * max, rounded once on the host)
__global__ void __launch_bounds__(kBlock) k_rf_mark_max(const double *ind, int64_t E, double threshold, uint8_t *marks)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    marks[e] = ind[e] >= threshold ? 1 : 0;
}

// ---- MAG_REFINE_TOP_FRACTION: keys that sort the largest indicator first (+ 0.0: -0.0 would sort as the largest value), a
// stable sort keeps equal values in element order
__global__ void __launch_bounds__(kBlock) k_rf_top_keys(const double *ind, int64_t E, uint64_t *key, uint32_t *val)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    key[e] = ~(uint64_t)__double_as_longlong(ind[e] + 0.0);
    val[e] = (uint32_t)e;
}

__global__ void __launch_bounds__(kBlock) k_rf_mark_top(const uint32_t *val, int64_t k, uint8_t *marks)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k) return;
    marks[val[i]] = 1;
}

// ---- marked edges: the longest edge of every marked element (split 1) or all three (split 3)
__global__ void __launch_bounds__(kBlock) k_rf_mark_edges(const uint8_t *marks, const int32_t *eid, const uint8_t *lng, int64_t E,
                                                          int split, uint32_t *flag, uint32_t *counters)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E || !marks[e]) return;
    atomicAdd(&counters[RF_MARKED], 1u);
    if (split == 3) {
        flag_set(&flag[eid[3 * e]]);
        flag_set(&flag[eid[3 * e + 1]]);
        flag_set(&flag[eid[3 * e + 2]]);
    } else {
        flag_set(&flag[eid[3 * e + lng[e]]]);
    }
}

// ---- one closure sweep: an element with a marked edge gets its longest edge marked.  `seen`: the flags as they were before the
// sweep (a copy: no write of this launch), so that what a sweep marks, and with it the number of sweeps, is the same in every run
__global__ void __launch_bounds__(kBlock) k_rf_sweep(const int32_t *eid, const uint8_t *lng, int64_t E, const uint32_t *seen,
                                                     uint32_t *flag, uint32_t *changed)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const int32_t id[3] = {eid[3 * e], eid[3 * e + 1], eid[3 * e + 2]};
    const uint32_t f[3] = {seen[id[0]], seen[id[1]], seen[id[2]]};
    const int L = lng[e];
    if ((f[0] | f[1] | f[2]) && !f[L]) {
        flag_set(&flag[id[L]]);
        flag_set(changed);
    }
}

// ---- children per element: one more than its marked edges (after the closure a marked edge implies a marked longest edge)
__global__ void __launch_bounds__(kBlock) k_rf_child_counts(const int32_t *eid, int64_t E, const uint32_t *flag, int32_t *cnt,
                                                            uint32_t *counters)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e > E) return;
    if (e == E) {
        cnt[E] = 0;
        return;
    }
    const int c = 1 + (int)(flag[eid[3 * e]] + flag[eid[3 * e + 1]] + flag[eid[3 * e + 2]]);
    cnt[e] = c;
    if (c > 1) atomicAdd(&counters[RF_SPLIT2 + (c - 2)], 1u);
}

__global__ void k_rf_sizes(const int32_t *mid, const int32_t *off, int64_t n3, int64_t E, uint32_t *counters)
{
    counters[RF_NEW_NODES] = (uint32_t)mid[n3];
    counters[RF_NEW_ELEMS] = (uint32_t)off[E];
}

// ---- new nodes: marked edge number r (mid[i], the scan of the flags) becomes node N + r, the midpoint of its edge with the
// interpolated constraint; mid[i] becomes the edge's node, -1 for an unmarked edge
__global__ void __launch_bounds__(kBlock) k_rf_emit_nodes(RefineTables t, RefinedMesh o)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= 3 * t.E) return;
    if (!t.flag[i]) {
        t.mid[i] = -1;
        return;
    }
    const int64_t r = t.mid[i], j = t.N + r;
    t.mid[i] = (int32_t)j;
    const uint64_t key = t.ekey[i];
    const int64_t lo = (int64_t)(key >> 32), hi = (int64_t)(key & 0xffffffffu);
    const double2 *xy = (const double2 *)t.xy;
    const double2 l = xy[lo], h = xy[hi];
    ((double2 *)o.xy)[j] = make_double2(0.5 * (l.x + h.x), 0.5 * (l.y + h.y));
    double u[2];
    uint8_t known[2];
    for (int d = 0; d < 2; ++d) {
        const bool both = t.u_known[2 * lo + d] && t.u_known[2 * hi + d];
        known[d] = both ? 1 : 0;
        u[d] = both ? 0.5 * (t.u_in[2 * lo + d] + t.u_in[2 * hi + d]) : 0.0;
    }
    o.u_known[2 * j] = known[0];
    o.u_known[2 * j + 1] = known[1];
    ((double2 *)o.u_in)[j] = make_double2(u[0], u[1]);
    ((double2 *)o.f_in)[j] = make_double2(0.0, 0.0);
    ((int2 *)o.node_parents)[r] = make_int2((int)lo, (int)hi);
}

// ---- new elements: element e's children at off[e] .. off[e + 1]
__global__ void __launch_bounds__(kBlock) k_rf_emit_elements(RefineTables t, RefinedMesh o)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= t.E) return;
    const int L = t.lng[e];
    const int k1 = L == 2 ? 0 : L + 1, k2 = k1 == 2 ? 0 : k1 + 1;
    const int32_t M = t.mid[t.eid[3 * e + L]];
    int64_t at = t.off[e];
    int32_t *c = o.conn + 3 * at;
    const auto put = [&](int32_t a, int32_t b, int32_t d) {
        c[0] = a;
        c[1] = b;
        c[2] = d;
        c += 3;
        o.elem_parent[at++] = (int32_t)e;
    };
    if (M < 0) { // no marked edge: verbatim, not rotated
        put(t.conn[3 * e], t.conn[3 * e + 1], t.conn[3 * e + 2]);
        return;
    }
    const int32_t p = t.conn[3 * e + L], q = t.conn[3 * e + k1], r = t.conn[3 * e + k2];
    const int32_t A = t.mid[t.eid[3 * e + k1]], B = t.mid[t.eid[3 * e + k2]];
    if (B >= 0) {
        put(p, M, B);
        put(B, M, r);
    } else {
        put(p, M, r);
    }
    if (A >= 0) {
        put(M, q, A);
        put(M, A, r);
    } else {
        put(M, q, r);
    }
}

// ---- launch wrappers
void refine_edge_keys(const RefineTables &t, hipStream_t s)
{
    k_rf_edge_keys<<<blocks_for(3 * t.E), kBlock, 0, s>>>(t.conn, 3 * t.E, t.key0, t.val0);
}

void refine_heads(const RefineTables &t, hipStream_t s) { k_rf_heads<<<blocks_for(3 * t.E), kBlock, 0, s>>>(t.key1, 3 * t.E, t.head); }

void refine_edge_table(const RefineTables &t, hipStream_t s)
{
    k_rf_edge_table<<<blocks_for(3 * t.E), kBlock, 0, s>>>(t.key1, t.val1, t.head, t.hscan, 3 * t.E, t.eid, t.ekey);
    k_rf_longest<<<blocks_for(t.E), kBlock, 0, s>>>((const double2 *)t.xy, t.conn, t.eid, t.E, t.lng);
}

void refine_check_indicator(const RefineTables &t, const double *ind, hipStream_t s)
{
    k_rf_check_indicator<<<blocks_for(t.E), kBlock, 0, s>>>(ind, t.E, t.check);
}

void refine_mark_max(const RefineTables &t, const double *ind, double threshold, hipStream_t s)
{
    k_rf_mark_max<<<blocks_for(t.E), kBlock, 0, s>>>(ind, t.E, threshold, t.marks);
}

void refine_top_keys(const RefineTables &t, const double *ind, hipStream_t s)
{
    k_rf_top_keys<<<blocks_for(t.E), kBlock, 0, s>>>(ind, t.E, t.key0, t.val0);
}

void refine_mark_top(const RefineTables &t, int64_t k, hipStream_t s) { k_rf_mark_top<<<blocks_for(k), kBlock, 0, s>>>(t.val1, k, t.marks); }

void refine_mark_edges(const RefineTables &t, int split, hipStream_t s)
{
    k_rf_mark_edges<<<blocks_for(t.E), kBlock, 0, s>>>(t.marks, t.eid, t.lng, t.E, split, t.flag, t.counters);
}

void refine_sweeps(const RefineTables &t, int sweeps, hipStream_t s)
{
    // (mid is free until the scan after the closure: it holds the flags a sweep reads)
    for (int j = 0; j < sweeps && j < kRefineSweepBatch; ++j) {
        (void)hipMemcpyAsync(t.mid, t.flag, 4 * (3 * (size_t)t.E + 1), hipMemcpyDeviceToDevice, s);
        k_rf_sweep<<<blocks_for(t.E), kBlock, 0, s>>>(t.eid, t.lng, t.E, (const uint32_t *)t.mid, t.flag, t.counters + RF_CHANGED + j);
    }
}

void refine_child_counts(const RefineTables &t, hipStream_t s)
{
    k_rf_child_counts<<<blocks_for(t.E + 1), kBlock, 0, s>>>(t.eid, t.E, t.flag, t.cnt, t.counters);
}

void refine_sizes(const RefineTables &t, hipStream_t s) { k_rf_sizes<<<1, 1, 0, s>>>(t.mid, t.off, 3 * t.E, t.E, t.counters); }

void refine_emit(const RefineTables &t, const RefinedMesh &out, hipStream_t s)
{
    k_rf_emit_nodes<<<blocks_for(3 * t.E), kBlock, 0, s>>>(t, out);
    k_rf_emit_elements<<<blocks_for(t.E), kBlock, 0, s>>>(t, out);
}

} // namespace magk
