// The bilinear pass of mag_run_adjoint: for solved members with displacements u and adjoint solutions lambda, the derivatives
// dJ/dtheta = -lambda^T (dK/dtheta) u with respect to an element-wise stiffness scale, every node coordinate, E, nu and the
// thickness, and dJ/d(loads).  The skeleton is sens.hip's: one pass over elements, one over nodes (tile by tile of the Hilbert
// order on an LDS image of the tile, or gathered from memory), a two-stage reduction of fixed shape -- per member, the member
// from blockIdx.y.  No floating-point atomics: a run gives the same bits every time and a member the same bits whatever
// launch it shares.  Compiled -ffp-contract=off: the rounding is the source's.
//
// With K_e = (B^T D) B A t (solver.rs:263-278), B's entries divided by 2A with the SIGNED area A, b and g as in sens.hip,
//   p_v = sum b_i vx_i,  q_v = sum g_i vy_i,  r_v = sum (g_i vx_i + b_i vy_i)    for v = u and v = l (lambda),
//   Qb = p_l p_u + q_l q_u + nu (p_l q_u + q_l p_u) + (1 - nu) / 2 r_l r_u,       A2 = 2A,  om = 1 - nu^2,
// the element's bilinear form is l_e^T K_e u_e = E t Qb / (2 A2 om) (Qb = Q of sens.hip where l = u: twice the energy); its
// derivatives follow in closed form as there.
#include "adjoint.h"

namespace magk {

namespace {

struct BilinearState {
    double pu, qu, ru, pl, ql, rl, A2;
};

// (coordinates, u and lambda of the element's corners in cyclic order starting anywhere: all seven are cyclic sums)
__device__ inline BilinearState bilinear_state(const double2 (&c)[3], const double2 (&u)[3], const double2 (&l)[3])
{
    const double b0 = c[1].y - c[2].y, b1 = c[2].y - c[0].y, b2 = c[0].y - c[1].y;
    const double g0 = c[2].x - c[1].x, g1 = c[0].x - c[2].x, g2 = c[1].x - c[0].x;
    BilinearState s;
    s.pu = b0 * u[0].x + b1 * u[1].x + b2 * u[2].x;
    s.qu = g0 * u[0].y + g1 * u[1].y + g2 * u[2].y;
    s.ru = (g0 * u[0].x + b0 * u[0].y) + (g1 * u[1].x + b1 * u[1].y) + (g2 * u[2].x + b2 * u[2].y);
    s.pl = b0 * l[0].x + b1 * l[1].x + b2 * l[2].x;
    s.ql = g0 * l[0].y + g1 * l[1].y + g2 * l[2].y;
    s.rl = (g0 * l[0].x + b0 * l[0].y) + (g1 * l[1].x + b1 * l[1].y) + (g2 * l[2].x + b2 * l[2].y);
    s.A2 = c[0].x * b0 + c[1].x * b1 + c[2].x * b2;
    return s;
}

__device__ inline double bilinear_Q(const BilinearState &s, double nu)
{
    return s.pl * s.pu + s.ql * s.qu + nu * (s.pl * s.qu + s.ql * s.pu) + 0.5 * (1.0 - nu) * s.rl * s.ru;
}

// the element's corners in cyclic order starting at corner m (selects, not an indexed array: nothing goes to scratch)
__device__ inline void load_corners(const double2 *xy, const double2 *u, const double2 *lam, const int32_t *conn, int64_t e, int m,
                                    double2 (&c)[3], double2 (&d)[3], double2 (&l)[3])
{
    const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
    const int32_t a = m == 0 ? n0 : (m == 1 ? n1 : n2), b = m == 0 ? n1 : (m == 1 ? n2 : n0), cc = m == 0 ? n2 : (m == 1 ? n0 : n1);
    c[0] = xy[a];
    c[1] = xy[b];
    c[2] = xy[cc];
    d[0] = u[a];
    d[1] = u[b];
    d[2] = u[cc];
    l[0] = lam[a];
    l[1] = lam[b];
    l[2] = lam[cc];
}

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

struct Member {
    const double2 *xy, *u, *lam;
    double youngs, nu, thick;
};

__device__ inline Member member_of(const AdjointBatch &ab, int64_t v, int64_t N)
{
    Member m;
    m.xy = (const double2 *)ab.xy + v * (ab.xy_stride / 2);
    m.u = (const double2 *)ab.u + v * N;
    m.lam = (const double2 *)ab.lam + v * N;
    m.youngs = ab.mat[ab.mat_stride * v];
    m.nu = ab.mat[ab.mat_stride * v + 1];
    m.thick = ab.mat[ab.mat_stride * v + 2];
    return m;
}

} // namespace

// ---- 1. per element: delem[e] = -l_e^T K_e u_e and l_e^T (dK_e / dnu) u_e
__global__ void __launch_bounds__(256) k_adjoint_elements(const int32_t *conn, int64_t N, int64_t E, AdjointBatch ab)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (e >= E) return;
    const Member m = member_of(ab, v, N);
    double2 c[3], d[3], l[3];
    load_corners(m.xy, m.u, m.lam, conn, e, 0, c, d, l);
    const BilinearState s = bilinear_state(c, d, l);
    const double Qb = bilinear_Q(s, m.nu), om = 1.0 - m.nu * m.nu;
    const double k = m.youngs * m.thick / (2.0 * s.A2);
    ab.delem[v * E + e] = -(k * Qb / om);
    // d/dnu of Qb / (1 - nu^2)
    ab.nuterm[v * E + e] = k * (((s.pl * s.qu + s.ql * s.pu) - 0.5 * s.rl * s.ru) / om + 2.0 * m.nu * Qb / (om * om));
}

// One corner's share of a node's sum: the derivative of l_e^T K_e u_e of the triangle (c, d, l: coordinates, u and lambda of its
// corners in cyclic order, corner 0 the node) with respect to the node's x and y, u and lambda held fixed.  cm = E t / (2 om).
__device__ inline void corner_bilinear(const double2 (&c)[3], const double2 (&d)[3], const double2 (&l)[3], double nu, double cm,
                                       double &gx, double &gy)
{
    const BilinearState s = bilinear_state(c, d, l);
    const double Qb = bilinear_Q(s, nu), ia = 1.0 / s.A2, h = 0.5 * (1.0 - nu);
    const double b0 = c[1].y - c[2].y, g0 = c[2].x - c[1].x;
    // x0 enters g1 (+) and g2 (-): dq_v = vy1 - vy2, dr_v = vx1 - vx2; y0 enters b1 (-) and b2 (+): dp_v = vx2 - vx1, dr_v = vy2 - vy1
    const double dQx = (s.ql + nu * s.pl) * (d[1].y - d[2].y) + (s.qu + nu * s.pu) * (l[1].y - l[2].y) +
                       h * ((l[1].x - l[2].x) * s.ru + s.rl * (d[1].x - d[2].x));
    const double dQy = (s.pl + nu * s.ql) * (d[2].x - d[1].x) + (s.pu + nu * s.qu) * (l[2].x - l[1].x) +
                       h * ((l[2].y - l[1].y) * s.ru + s.rl * (d[2].y - d[1].y));
    gx += cm * ia * (dQx - Qb * b0 * ia);
    gy += cm * ia * (dQy - Qb * g0 * ia);
}

// ---- 2. per node: dxy[2i + d] = -(sum over the node's incident triangles, in the order of its incidence list, of the derivative
// of l_e^T K_e u_e with respect to coordinate d of the node).  One workgroup per tile of the Hilbert order and member, as
// k_sens_nodes_tile: the tile's image -- coordinates, u and lambda of its owned and halo nodes, each fetched once through perm
// -- is staged in LDS, the triangles come from the tile-local table.  Dynamic LDS: 48 * cap bytes, up to 96768 at
// cap = kMaxLdsNodes (one workgroup per CU then, one wave per SIMD; the launch wrapper raises the 64 KiB default limit).
// Three planes of double2 rather than one 48-byte record: a wave's 16-byte reads of one plane then start at multiples of 16.
__global__ void __launch_bounds__(256) k_adjoint_nodes_tile(const uint32_t *perm, const int32_t *halo_g, const int32_t *tile_hoff,
                                                             const int32_t *tile_deg, const int64_t *tile_off, const uint32_t *tab,
                                                             int64_t N, int32_t B, int32_t cap, AdjointBatch ab)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    double2 *s_xy = s_img, *s_u = s_img + cap, *s_l = s_img + 2 * cap; // [cap] each: owned nodes 0 .. B-1, halo nodes from B
    const int32_t t = blockIdx.x;
    const int64_t v = blockIdx.y, base = (int64_t)t * B;
    const Member m = member_of(ab, v, N);
    const int32_t hoff = tile_hoff[t], nh = tile_hoff[t + 1] - hoff; // B + nh <= cap
    for (int32_t l = threadIdx.x; l < B; l += 256)
        if (base + l < N) {
            const uint32_t id = perm[base + l];
            s_xy[l] = m.xy[id];
            s_u[l] = m.u[id];
            s_l[l] = m.lam[id];
        }
    for (int32_t h = threadIdx.x; h < nh; h += 256) {
        const uint32_t id = perm[halo_g[hoff + h]];
        s_xy[B + h] = m.xy[id];
        s_u[B + h] = m.u[id];
        s_l[B + h] = m.lam[id];
    }
    __syncthreads();
    const double cm = m.youngs * m.thick / (2.0 * (1.0 - m.nu * m.nu));
    const int32_t td = tile_deg[t];
    const uint32_t *table = tab + tile_off[t];
    for (int32_t l = threadIdx.x; l < B; l += 256) {
        if (base + l >= N) break;
        double2 c[3], d[3], a[3];
        c[0] = s_xy[l];
        d[0] = s_u[l];
        a[0] = s_l[l];
        double gx = 0.0, gy = 0.0;
        for (int32_t k = 0; k < td; ++k) {
            const uint32_t w = table[(int64_t)k * B + l];
            if (w == 0xffffffffu) break; // (a node's words are its list's, in order, then the filler)
            const uint32_t lb = w & 0xffffu, lc = w >> 16;
            c[1] = s_xy[lb];
            c[2] = s_xy[lc];
            d[1] = s_u[lb];
            d[2] = s_u[lc];
            a[1] = s_l[lb];
            a[2] = s_l[lc];
            corner_bilinear(c, d, a, m.nu, cm, gx, gy);
        }
        ((double2 *)ab.dxy)[v * N + perm[base + l]] = make_double2(-gx, -gy);
    }
}

// ---- ... the same sums gathered from memory (a tile image too large for the LDS, or MAG_TUNE_SENS_STAGE=0): lane g takes node
// perm[g], inc[k] = 3e + (corner of e that is this node), ascending per node.  The same arithmetic in the same order: the same bits.
__global__ void __launch_bounds__(256) k_adjoint_nodes(const int32_t *inc_off, const uint32_t *inc, const uint32_t *perm,
                                                        const int32_t *conn, int64_t N, AdjointBatch ab)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (g >= N) return;
    const Member m = member_of(ab, v, N);
    const double cm = m.youngs * m.thick / (2.0 * (1.0 - m.nu * m.nu));
    double gx = 0.0, gy = 0.0;
    const int32_t k1 = inc_off[g + 1];
    for (int32_t k = inc_off[g]; k < k1; ++k) {
        const uint32_t w = inc[k];
        const int64_t e = w / 3u;
        double2 c[3], d[3], a[3];
        load_corners(m.xy, m.u, m.lam, conn, e, (int)(w - 3u * (uint32_t)e), c, d, a); // corner 0 is this node
        corner_bilinear(c, d, a, m.nu, cm, gx, gy);
    }
    ((double2 *)ab.dxy)[v * N + perm[g]] = make_double2(-gx, -gy);
}

// ---- 3. per DOF: dJ/df_in = lambda on a free DOF, dJ/du_in = g - (K lambda) on a prescribed one
__global__ void __launch_bounds__(256) k_adjoint_dloads(const uint8_t *u_known, int64_t N, AdjointBatch ab)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, at = (int64_t)blockIdx.y * 2 * N + i;
    if (i >= 2 * N) return;
    ab.dloads[at] = u_known[i] ? ab.g[at] - ab.f_adj[at] : ab.lam[at];
}

// ---- 4. scalars, stage one: kSensBlocks workgroups per member, each over a fixed share of the elements
__global__ void __launch_bounds__(256) k_adjoint_partials(int64_t E, AdjointBatch ab)
{
    __shared__ double s_red[8];
    const int64_t v = blockIdx.y, first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)kSensBlocks * 256;
    const double *delem = ab.delem + v * E, *nuterm = ab.nuterm + v * E;
    double acc[2] = {0.0, 0.0}; // sum of delem, sum of the nu terms
    for (int64_t e = first; e < E; e += step) {
        acc[0] += delem[e];
        acc[1] += nuterm[e];
    }
    block_sum256<2>(acc, s_red);
    if (threadIdx.x == 0) {
        double *out = ab.partials + 2 * ((int64_t)kSensBlocks * v + blockIdx.x);
        out[0] = acc[0];
        out[1] = acc[1];
    }
}

// ---- ... stage two: one workgroup per member over its kSensBlocks partial records
__global__ void __launch_bounds__(256) k_adjoint_scalars(AdjointBatch ab)
{
    static_assert(kSensBlocks == 256, "one partial record per thread");
    __shared__ double s_red[8];
    const int64_t v = blockIdx.y;
    const double *in = ab.partials + 2 * ((int64_t)kSensBlocks * v + threadIdx.x);
    double acc[2] = {in[0], in[1]};
    block_sum256<2>(acc, s_red);
    if (threadIdx.x != 0) return;
    double *out = ab.scalars + 8 * v;
    out[0] = -acc[0]; // a = sum of l_e^T K_e u_e
    out[1] = acc[0] / ab.mat[ab.mat_stride * v];
    out[2] = -acc[1];
    out[3] = acc[0] / ab.mat[ab.mat_stride * v + 2];
    out[4] = out[5] = out[6] = out[7] = 0.0;
}

hipError_t adjoint_bilinear(const SensMesh &m, const AdjointBatch &ab, hipStream_t s)
{
    const unsigned n = (unsigned)ab.count;
    const int64_t N = m.N, E = m.E;
    k_adjoint_elements<<<dim3((unsigned)((E + 255) / 256), n), 256, 0, s>>>(m.conn, N, E, ab);
    if (m.tab) {
        const size_t lds = 48 * (size_t)m.cap; // cap <= kMaxLdsNodes: at most 96768 of the CU's 160 KiB
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute((const void *)k_adjoint_nodes_tile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        k_adjoint_nodes_tile<<<dim3((unsigned)m.T, n), 256, lds, s>>>(m.perm, m.halo_g, m.tile_hoff, m.tile_deg, m.tile_off, m.tab, N,
                                                                     m.B, m.cap, ab);
    } else {
        k_adjoint_nodes<<<dim3((unsigned)((N + 255) / 256), n), 256, 0, s>>>(m.inc_off, m.inc, m.perm, m.conn, N, ab);
    }
    k_adjoint_dloads<<<dim3((unsigned)((2 * N + 255) / 256), n), 256, 0, s>>>(m.u_known, N, ab);
    k_adjoint_partials<<<dim3(kSensBlocks, n), 256, 0, s>>>(E, ab);
    k_adjoint_scalars<<<dim3(1, n), 256, 0, s>>>(ab);
    return hipSuccess;
}

} // namespace magk
