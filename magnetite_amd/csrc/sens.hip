// Energy and design sensitivities of solved members (mag_run_sensitivities): strain energy per element, its gradient with
// respect to every node coordinate, and the scalar objective terms.  One pass over elements, one over nodes, a two-stage
// reduction -- per member, the member taken from blockIdx.y as the _v kernels of exact.hip do.  Everything is in the caller's
// numbering; the node kernel works tile by tile of the Hilbert order on an LDS image of the tile.  No floating-point atomics: every sum has a fixed shape, a run gives the same bits every time and a
// member the same bits whatever launch it shares.  Compiled -ffp-contract=off: the rounding is the source's.
//
// With K_e = (B^T D) B A t (solver.rs:263-278), B's entries divided by 2A with the SIGNED area A, and
//   p = sum b_i ux_i,  q = sum g_i uy_i,  r = sum (g_i ux_i + b_i uy_i),   b = (y1-y2, y2-y0, y0-y1), g = (x2-x1, x0-x2, x1-x0),
//   Q = p^2 + q^2 + 2 nu p q + (1 - nu) / 2 r^2,      A2 = 2A = sum x_i b_i,
// the element's energy is 1/2 u_e^T K_e u_e = E t Q / (4 A2 (1 - nu^2)); its derivatives follow in closed form.
#include "sens.h"

namespace magk {

namespace {

struct ElemState {
    double p, q, r, A2;
};

// (x, y, ux, uy of the element's corners in cyclic order starting anywhere: p, q, r and A2 are cyclic sums)
__device__ inline ElemState elem_state(const double2 (&c)[3], const double2 (&u)[3])
{
    const double b0 = c[1].y - c[2].y, b1 = c[2].y - c[0].y, b2 = c[0].y - c[1].y;
    const double g0 = c[2].x - c[1].x, g1 = c[0].x - c[2].x, g2 = c[1].x - c[0].x;
    ElemState s;
    s.p = b0 * u[0].x + b1 * u[1].x + b2 * u[2].x;
    s.q = g0 * u[0].y + g1 * u[1].y + g2 * u[2].y;
    s.r = (g0 * u[0].x + b0 * u[0].y) + (g1 * u[1].x + b1 * u[1].y) + (g2 * u[2].x + b2 * u[2].y);
    s.A2 = c[0].x * b0 + c[1].x * b1 + c[2].x * b2;
    return s;
}

__device__ inline double elem_Q(const ElemState &s, double nu)
{
    return s.p * s.p + s.q * s.q + 2.0 * nu * s.p * s.q + 0.5 * (1.0 - nu) * s.r * s.r;
}

// the element's corners in cyclic order starting at corner m (selects, not an indexed array: nothing goes to scratch)
__device__ inline void load_corners(const double2 *xy, const double2 *u, const int32_t *conn, int64_t e, int m, double2 (&c)[3],
                                    double2 (&d)[3])
{
    const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
    const int32_t a = m == 0 ? n0 : (m == 1 ? n1 : n2), b = m == 0 ? n1 : (m == 1 ? n2 : n0), cc = m == 0 ? n2 : (m == 1 ? n0 : n1);
    c[0] = xy[a];
    c[1] = xy[b];
    c[2] = xy[cc];
    d[0] = u[a];
    d[1] = u[b];
    d[2] = u[cc];
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

} // namespace

// ---- 1. per element: energy[e] = 1/2 u_e^T K_e u_e and d(energy[e]) / d(nu)
__global__ void __launch_bounds__(256) k_sens_energy(const int32_t *conn, int64_t N, int64_t E, SensBatch sb)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (e >= E) return;
    const double2 *xy = (const double2 *)sb.xy + v * (sb.xy_stride / 2), *u = (const double2 *)sb.u + v * N;
    const double youngs = sb.mat[sb.mat_stride * v], nu = sb.mat[sb.mat_stride * v + 1], thick = sb.mat[sb.mat_stride * v + 2];
    double2 c[3], d[3];
    load_corners(xy, u, conn, e, 0, c, d);
    const ElemState s = elem_state(c, d);
    const double Q = elem_Q(s, nu), om = 1.0 - nu * nu;
    const double k = youngs * thick / (4.0 * s.A2);
    sb.energy[v * E + e] = k * Q / om;
    // d/dnu of Q / (1 - nu^2)
    sb.nuterm[v * E + e] = k * ((2.0 * s.p * s.q - 0.5 * s.r * s.r) / om + 2.0 * nu * Q / (om * om));
}

// One corner's share of a node's gradient: the derivative of the energy of the triangle (c, d: coordinates and displacements
// of its corners in cyclic order, corner 0 the node) with respect to the node's x and y, u held fixed.
__device__ inline void corner_gradient(const double2 (&c)[3], const double2 (&d)[3], double nu, double cm, double &gx, double &gy)
{
    const ElemState s = elem_state(c, d);
    const double Q = elem_Q(s, nu), ia = 1.0 / s.A2;
    const double b0 = c[1].y - c[2].y, g0 = c[2].x - c[1].x;
    // x0 enters g1 (+) and g2 (-): dq = uy1 - uy2, dr = ux1 - ux2; y0 enters b1 (-) and b2 (+): dp = ux2 - ux1, dr = uy2 - uy1
    const double dQx = 2.0 * (s.q + nu * s.p) * (d[1].y - d[2].y) + (1.0 - nu) * s.r * (d[1].x - d[2].x);
    const double dQy = 2.0 * (s.p + nu * s.q) * (d[2].x - d[1].x) + (1.0 - nu) * s.r * (d[2].y - d[1].y);
    gx += cm * ia * (dQx - Q * b0 * ia);
    gy += cm * ia * (dQy - Q * g0 * ia);
}

// ---- 2. per node: dxy[2i + d] = sum over the node's incident triangles, in the order of its incidence list, of the
// triangle's energy derivative with respect to coordinate d of the node (u held fixed).  A gather, one workgroup per tile of
// the Hilbert order and member.  The tile's image -- coordinates and displacements of its owned and halo nodes, each fetched
// once from the member's caller-order arrays through perm -- is staged in LDS as k_assemble_fan stages coordinates; the
// triangles then come from the tile-local table (tab: word k of node l = the two OTHER corners of the node's k-th triangle as
// tile-local ids, lb | lc << 16, 0xffffffff past the node's last: fill_ell16's first form), read coalesced, and every corner
// from LDS.  Dynamic LDS: 32 * cap bytes.
__global__ void __launch_bounds__(256) k_sens_nodes_tile(const uint32_t *perm, const int32_t *halo_g, const int32_t *tile_hoff,
                                                          const int32_t *tile_deg, const int64_t *tile_off, const uint32_t *tab,
                                                          int64_t N, int32_t B, int32_t cap, SensBatch sb)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    double2 *s_xy = s_img, *s_u = s_img + cap; // [cap] each: owned nodes 0 .. B-1, halo nodes from B
    const int32_t t = blockIdx.x;
    const int64_t v = blockIdx.y, base = (int64_t)t * B;
    const double2 *xy = (const double2 *)sb.xy + v * (sb.xy_stride / 2), *u = (const double2 *)sb.u + v * N;
    const int32_t hoff = tile_hoff[t], nh = tile_hoff[t + 1] - hoff; // B + nh <= cap
    for (int32_t l = threadIdx.x; l < B; l += 256)
        if (base + l < N) {
            const uint32_t id = perm[base + l];
            s_xy[l] = xy[id];
            s_u[l] = u[id];
        }
    for (int32_t h = threadIdx.x; h < nh; h += 256) {
        const uint32_t id = perm[halo_g[hoff + h]];
        s_xy[B + h] = xy[id];
        s_u[B + h] = u[id];
    }
    __syncthreads();
    const double youngs = sb.mat[sb.mat_stride * v], nu = sb.mat[sb.mat_stride * v + 1], thick = sb.mat[sb.mat_stride * v + 2];
    const double cm = youngs * thick / (4.0 * (1.0 - nu * nu));
    const int32_t td = tile_deg[t];
    const uint32_t *table = tab + tile_off[t];
    for (int32_t l = threadIdx.x; l < B; l += 256) {
        if (base + l >= N) break;
        double2 c[3], d[3];
        c[0] = s_xy[l];
        d[0] = s_u[l];
        double gx = 0.0, gy = 0.0;
        for (int32_t k = 0; k < td; ++k) {
            const uint32_t w = table[(int64_t)k * B + l];
            if (w == 0xffffffffu) break; // (a node's words are its list's, in order, then the filler)
            const uint32_t lb = w & 0xffffu, lc = w >> 16;
            c[1] = s_xy[lb];
            c[2] = s_xy[lc];
            d[1] = s_u[lb];
            d[2] = s_u[lc];
            corner_gradient(c, d, nu, cm, gx, gy);
        }
        ((double2 *)sb.dxy)[v * N + perm[base + l]] = make_double2(gx, gy);
    }
}

// ---- ... the same sums for a mesh whose tile image does not fit the LDS (cap > kMaxLdsNodes: no tile-local table either):
// lane g takes node perm[g] and gathers every corner from memory.  inc[k] = 3e + (corner of e that is this node), ascending
// per node.  The same arithmetic in the same order: the same bits.
__global__ void __launch_bounds__(256) k_sens_nodes(const int32_t *inc_off, const uint32_t *inc, const uint32_t *perm,
                                                     const int32_t *conn, int64_t N, SensBatch sb)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (g >= N) return;
    const double2 *xy = (const double2 *)sb.xy + v * (sb.xy_stride / 2), *u = (const double2 *)sb.u + v * N;
    const double youngs = sb.mat[sb.mat_stride * v], nu = sb.mat[sb.mat_stride * v + 1], thick = sb.mat[sb.mat_stride * v + 2];
    const double cm = youngs * thick / (4.0 * (1.0 - nu * nu));
    double gx = 0.0, gy = 0.0;
    const int32_t k1 = inc_off[g + 1];
    for (int32_t k = inc_off[g]; k < k1; ++k) {
        const uint32_t w = inc[k];
        const int64_t e = w / 3u;
        double2 c[3], d[3];
        load_corners(xy, u, conn, e, (int)(w - 3u * (uint32_t)e), c, d); // corner 0 is this node
        corner_gradient(c, d, nu, cm, gx, gy);
    }
    ((double2 *)sb.dxy)[v * N + perm[g]] = make_double2(gx, gy);
}

// ---- 3. scalars, stage one: kSensBlocks workgroups per member, each over a fixed share of the elements and the DOFs
__global__ void __launch_bounds__(256) k_sens_partials(const uint8_t *u_known, int64_t N, int64_t E, SensBatch sb)
{
    __shared__ double s_red[16];
    const int64_t v = blockIdx.y, first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)kSensBlocks * 256;
    const double *energy = sb.energy + v * E, *nuterm = sb.nuterm + v * E;
    const double *u = sb.u + v * 2 * N, *f = sb.f_out + v * 2 * N;
    const double *u_in = sb.u_in + v * sb.loads_stride, *f_in = sb.f_in + v * sb.loads_stride;
    double acc[4] = {0.0, 0.0, 0.0, 0.0}; // W, dW/dnu, external work, reaction work
    for (int64_t e = first; e < E; e += step) {
        acc[0] += energy[e];
        acc[1] += nuterm[e];
    }
    for (int64_t i = first; i < 2 * N; i += step) {
        if (u_known[i])
            acc[3] += f[i] * u_in[i];
        else
            acc[2] += f_in[i] * u[i];
    }
    block_sum256<4>(acc, s_red);
    if (threadIdx.x == 0) {
        double *out = sb.partials + 4 * ((int64_t)kSensBlocks * v + blockIdx.x);
        for (int c = 0; c < 4; ++c) out[c] = acc[c];
    }
}

// ---- ... stage two: one workgroup per member over its kSensBlocks partial records
__global__ void __launch_bounds__(256) k_sens_scalars(SensBatch sb)
{
    static_assert(kSensBlocks == 256, "one partial record per thread");
    __shared__ double s_red[16];
    const int64_t v = blockIdx.y;
    const double *in = sb.partials + 4 * ((int64_t)kSensBlocks * v + threadIdx.x);
    double acc[4] = {in[0], in[1], in[2], in[3]};
    block_sum256<4>(acc, s_red);
    if (threadIdx.x != 0) return;
    double *out = sb.scalars + 8 * v;
    const double W = acc[0];
    out[0] = W;
    out[1] = W - acc[2];
    out[2] = acc[2];
    out[3] = acc[3];
    out[4] = W / sb.mat[sb.mat_stride * v];
    out[5] = acc[1];
    out[6] = W / sb.mat[sb.mat_stride * v + 2];
    out[7] = 0.0;
}

void sensitivities(const SensMesh &m, const SensBatch &sb, hipStream_t s)
{
    const unsigned n = (unsigned)sb.count;
    const int64_t N = m.N, E = m.E;
    k_sens_energy<<<dim3((unsigned)((E + 255) / 256), n), 256, 0, s>>>(m.conn, N, E, sb);
    if (m.tab)
        k_sens_nodes_tile<<<dim3((unsigned)m.T, n), 256, 32 * (size_t)m.cap, s>>>(m.perm, m.halo_g, m.tile_hoff, m.tile_deg, m.tile_off,
                                                                                  m.tab, N, m.B, m.cap, sb);
    else
        k_sens_nodes<<<dim3((unsigned)((N + 255) / 256), n), 256, 0, s>>>(m.inc_off, m.inc, m.perm, m.conn, N, sb);
    k_sens_partials<<<dim3(kSensBlocks, n), 256, 0, s>>>(m.u_known, N, E, sb);
    k_sens_scalars<<<dim3(1, n), 256, 0, s>>>(sb);
}

} // namespace magk
