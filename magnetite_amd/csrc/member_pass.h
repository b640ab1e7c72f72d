// Internal, device code: the skeleton of a pass over the solved members of a set, shared by sens.hip, adjoint.hip and
// objective.hip -- one pass over elements, one over nodes (tile by tile of the Hilbert order on an LDS image of the tile, or
// gathered from memory), a two-stage reduction of fixed shape; per member, the member from blockIdx.y.  No floating-point
// atomics: every sum has a fixed shape, a run gives the same bits every time and a member the same bits whatever launch it
// shares.  The three files are compiled -ffp-contract=off: the rounding is this source's, nothing here may be reassociated.
#pragma once
#include "sens.h"

namespace magk {

// ---- the member v of a batch
struct Member {
    const double2 *xy, *u;
    double youngs, nu, thick;
    const double *scale; // per element, or null
};

__device__ inline Member member_of(const MemberBatch &mb, int64_t v, int64_t N)
{
    Member m;
    m.xy = (const double2 *)mb.xy + v * (mb.xy_stride / 2);
    m.u = (const double2 *)mb.u + v * N;
    m.youngs = mb.mat[mb.mat_stride * v];
    m.nu = mb.mat[mb.mat_stride * v + 1];
    m.thick = mb.mat[mb.mat_stride * v + 2];
    m.scale = mb.scale;
    return m;
}

// ---- a triangle's edge differences and the cyclic sums over them.  With K_e = (B^T D) B A t (solver.rs:263-278), B's entries
// divided by 2A with the SIGNED area A:  b = (y1-y2, y2-y0, y0-y1), g = (x2-x1, x0-x2, x1-x0), A2 = 2A = sum x_i b_i, and for a
// vector field v on the corners  p = sum b_i vx_i,  q = sum g_i vy_i,  r = sum (g_i vx_i + b_i vy_i).
struct Edges {
    double b[3], g[3], A2;
};

struct Sums {
    double p, q, r;
};

// (the corners in cyclic order starting anywhere: A2 is a cyclic sum, and so are p, q, r)
__device__ inline Edges edges_of(const double2 (&c)[3])
{
    Edges e;
    e.b[0] = c[1].y - c[2].y, e.b[1] = c[2].y - c[0].y, e.b[2] = c[0].y - c[1].y;
    e.g[0] = c[2].x - c[1].x, e.g[1] = c[0].x - c[2].x, e.g[2] = c[1].x - c[0].x;
    e.A2 = c[0].x * e.b[0] + c[1].x * e.b[1] + c[2].x * e.b[2];
    return e;
}

__device__ inline Sums cyclic_sums(const Edges &e, const double2 (&v)[3])
{
    Sums s;
    s.p = e.b[0] * v[0].x + e.b[1] * v[1].x + e.b[2] * v[2].x;
    s.q = e.g[0] * v[0].y + e.g[1] * v[1].y + e.g[2] * v[2].y;
    s.r = (e.g[0] * v[0].x + e.b[0] * v[0].y) + (e.g[1] * v[1].x + e.b[1] * v[1].y) + (e.g[2] * v[2].x + e.b[2] * v[2].y);
    return s;
}

// ---- P fields (coordinates, u, ...) of element e's corners in cyclic order starting at corner m (selects, not an indexed
// array: nothing goes to scratch)
template <int P>
__device__ inline void load_corners(const double2 *const (&src)[P], const int32_t *conn, int64_t e, int m, double2 (&f)[P][3])
{
    const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
    const int32_t a = m == 0 ? n0 : (m == 1 ? n1 : n2), b = m == 0 ? n1 : (m == 1 ? n2 : n0), cc = m == 0 ? n2 : (m == 1 ? n0 : n1);
#pragma unroll
    for (int j = 0; j < P; ++j) {
        f[j][0] = src[j][a];
        f[j][1] = src[j][b];
        f[j][2] = src[j][cc];
    }
}

// ---- the pass over nodes.  A pass (sens.hip's Gradient, adjoint.hip's Bilinear, objective.hip's Stress) supplies
//   Node               what it sums per node,
//   node(pos)          the sums' start for the node at Hilbert position pos,
//   corner(n, f, k)    what the node's k-th incident triangle adds: f[j] = field j of its corners in cyclic order, corner 0 the
//                      node; the triangle's id, where the pass wants it, is inc[inc_off[pos] + k] / 3,
//   store(n, at)       what is written for the node, at = (member) * N + (caller id).
// ScaledCorners is what a pass whose terms carry the element stiffness field derives from: node(pos) keeps the node's incidence
// list, factor(n, k, cm) is cm times the scale of the node's k-th triangle -- cm itself where there is no field.
// Sums run in the order of the node's incidence list in both walks, with the same arithmetic: the same bits.

struct ScaledCorners {
    const double *scale;
    const uint32_t *inc;
    const int32_t *inc_off;
    struct Node {
        double gx, gy;
        const uint32_t *list;
    };
    __device__ ScaledCorners(const Member &m, const SensMesh &mesh) : scale(m.scale), inc(mesh.inc), inc_off(mesh.inc_off) {}
    __device__ Node node(int64_t pos) const { return {0.0, 0.0, scale ? inc + inc_off[pos] : nullptr}; }
    __device__ double factor(const Node &n, int32_t k, double cm) const { return scale ? cm * scale[n.list[k] / 3u] : cm; }
};

// One workgroup per tile of the Hilbert order and member (grid: T x count, 256 threads).  The tile's image -- P fields of its
// owned and halo nodes, each fetched once from the member's caller-order arrays through perm -- is staged in s_img as P planes
// of [cap] (owned nodes 0 .. B-1, halo nodes from B; planes rather than one record per node: a wave's 16-byte reads of one plane
// start at multiples of 16), as k_assemble_fan stages coordinates.  The triangles then come from the tile-local table (tab: word k
// of node l = the two OTHER corners of the node's k-th triangle as tile-local ids, lb | lc << 16, 0xffffffff past the node's
// last: fill_ell16's first form), read coalesced, and every corner from LDS.  Dynamic LDS: 16 * P * cap bytes.
template <int P, class Pass>
__device__ inline void tile_walk(const SensMesh &m, const double2 *const (&src)[P], double2 *s_img, const Pass &pass)
{
    const int32_t t = blockIdx.x, B = m.B, cap = m.cap;
    const int64_t v = blockIdx.y, N = m.N, base = (int64_t)t * B;
    const int32_t hoff = m.tile_hoff[t], nh = m.tile_hoff[t + 1] - hoff; // B + nh <= cap
    for (int32_t l = threadIdx.x; l < B; l += 256)
        if (base + l < N) {
            const uint32_t id = m.perm[base + l];
#pragma unroll
            for (int j = 0; j < P; ++j) s_img[j * cap + l] = src[j][id];
        }
    for (int32_t h = threadIdx.x; h < nh; h += 256) {
        const uint32_t id = m.perm[m.halo_g[hoff + h]];
#pragma unroll
        for (int j = 0; j < P; ++j) s_img[j * cap + B + h] = src[j][id];
    }
    __syncthreads();
    const int32_t td = m.tile_deg[t];
    const uint32_t *table = m.tab + m.tile_off[t];
    for (int32_t l = threadIdx.x; l < B; l += 256) {
        if (base + l >= N) break;
        double2 f[P][3];
#pragma unroll
        for (int j = 0; j < P; ++j) f[j][0] = s_img[j * cap + l];
        typename Pass::Node n = pass.node(base + l);
        for (int32_t k = 0; k < td; ++k) {
            const uint32_t w = table[(int64_t)k * B + l];
            if (w == 0xffffffffu) break; // (a node's words are its list's, in order, then the filler)
            const uint32_t lb = w & 0xffffu, lc = w >> 16;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                f[j][1] = s_img[j * cap + lb];
                f[j][2] = s_img[j * cap + lc];
            }
            pass.corner(n, f, k);
        }
        pass.store(n, v * N + m.perm[base + l]);
    }
}

// The same sums gathered from memory (a tile image too large for the LDS -- cap > kMaxLdsNodes: no tile-local table either -- or
// MAG_TUNE_SENS_STAGE=0): lane g takes the node at Hilbert position g (grid: ceil(N / 256) x count) and fetches every corner
// through conn.  inc[k] = 3e + (corner of e that is this node), ascending per node.
template <int P, class Pass>
__device__ inline void gather_walk(const SensMesh &m, const double2 *const (&src)[P], const Pass &pass)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (g >= m.N) return;
    typename Pass::Node n = pass.node(g);
    const uint32_t *list = m.inc + m.inc_off[g];
    const int32_t len = m.inc_off[g + 1] - m.inc_off[g];
    for (int32_t k = 0; k < len; ++k) {
        const uint32_t w = list[k];
        const int64_t e = w / 3u;
        double2 f[P][3];
        load_corners(src, m.conn, e, (int)(w - 3u * (uint32_t)e), f); // corner 0 is this node
        pass.corner(n, f, k);
    }
    pass.store(n, v * m.N + m.perm[g]);
}

// ---- the scalars: a two-stage reduction of NS sums per member, of a fixed shape whatever the mesh

// sum over the 256 threads of a workgroup of NS values each, in a fixed tree; the totals are valid in thread 0
template <int NS>
__device__ inline void block_sum256(double (&v)[NS], double *s_red)
{
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int c = 0; c < NS; ++c) v[c] += __shfl_down(v[c], off);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < NS; ++c) s_red[NS * w + c] = v[c];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < NS; ++c) v[c] = (s_red[c] + s_red[NS + c]) + (s_red[2 * NS + c] + s_red[3 * NS + c]);
}

// maximum over the 256 threads of a workgroup of NS values each, in block_sum256's shape; valid in thread 0
template <int NS>
__device__ inline void block_max256(double (&v)[NS], double *s_red)
{
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int c = 0; c < NS; ++c) v[c] = fmax(v[c], __shfl_down(v[c], off));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < NS; ++c) s_red[NS * w + c] = v[c];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < NS; ++c) v[c] = fmax(fmax(s_red[c], s_red[NS + c]), fmax(s_red[2 * NS + c], s_red[3 * NS + c]));
}

// Stage one (grid: kSensBlocks x count, 256 threads): every thread adds the pass's summands add(i, acc) of its fixed share of
// the n entries ...
template <int NS, class Add>
__device__ inline void share_sum(int64_t n, double (&acc)[NS], const Add &add)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kSensBlocks * 256) add(i, acc);
}

// ... and the workgroup leaves its sums as record blockIdx.x of the member's kSensBlocks in partials [count][kSensBlocks][NS]
template <int NS>
__device__ inline void store_partials(double (&acc)[NS], double *partials)
{
    __shared__ double s_red[4 * NS];
    block_sum256<NS>(acc, s_red);
    if (threadIdx.x == 0) {
        double *out = partials + NS * ((int64_t)kSensBlocks * blockIdx.y + blockIdx.x);
#pragma unroll
        for (int c = 0; c < NS; ++c) out[c] = acc[c];
    }
}

// Stage two (grid: 1 x count, 256 threads): one workgroup per member sums its kSensBlocks records; thread 0 hands the totals
// to the pass's finish(v, acc)
template <int NS, class Finish>
__device__ inline void sum_partials(const double *partials, const Finish &finish)
{
    static_assert(kSensBlocks == 256, "one partial record per thread");
    __shared__ double s_red[4 * NS];
    const int64_t v = blockIdx.y;
    const double *in = partials + NS * ((int64_t)kSensBlocks * v + threadIdx.x);
    double acc[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = in[c];
    block_sum256<NS>(acc, s_red);
    if (threadIdx.x == 0) finish(v, acc);
}

} // namespace magk
