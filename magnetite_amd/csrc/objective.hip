// Objectives of solved members on the device (mag_run_objective): J, g = dJ/du and J's explicit partials at fixed u -- what the
// adjoint pass (mag_run_adjoint) takes and what the caller would otherwise add to its results.  The skeleton is sens.hip's: one
// pass over elements, a two-stage reduction of fixed shape, one pass over nodes (tile by tile of the Hilbert order on an LDS
// image of the tile, or gathered from memory) -- per member, the member from blockIdx.y.  No floating-point atomics: a run gives
// the same bits every time and a member the same bits whatever launch it shares.  Compiled -ffp-contract=off: the rounding is
// the source's.
//
// MAG_OBJ_STRESS_PNORM.  sigma_e = D B u_e with the reference's D, B and SIGNED area (d_element_stress, exact.hip).  In the
// notation of sens.hip, p_u = sum b_i ux_i, q_u = sum g_i uy_i, r_u = sum (g_i ux_i + b_i uy_i), A2 = 2A, and with
//   P = p_u + nu q_u,  Q = nu p_u + q_u,  R = (1 - nu) / 2 r_u,  cs = E / (1 - nu^2):   (sx, sy, txy) = cs / A2 (P, Q, R),
//   M = P^2 - P Q + Q^2 + 3 R^2,      vm_e^2 = (cs / A2)^2 M.
// S = sum_e w_e (vm_e / scale)^ex, J = scale S^(1/ex).  With h_e = w_e (vm_e / scale)^(ex - 2) and F = S^(1/ex - 1) / (2 scale),
//   dJ/dz = F sum_e h_e d(vm_e^2)/dz                      for z = a displacement, a coordinate (u fixed), nu (u fixed),
// and d(vm_e^2)/dz follows in closed form from mP = dM/dP = 2P - Q, mQ = dM/dQ = 2Q - P, mR = dM/dR (1 - nu) / 2 = 3 (1 - nu) R.
// An element with vm_e = 0 has h_e = 0: it contributes nothing to S, g or the partials.
//
// MAG_OBJ_DISP_LSQ.  J = sum_i w_i (u_i - target_i)^2, g = 2 w (u - target); no explicit partial.
#include "objective.h"

namespace magk {

namespace {

struct StressState {
    double pu, qu, ru, A2;   // sens.hip's p, q, r, 2A
    double P, Q, R, M;       // as above
    double mP, mQ, mR;       // dM/dP, dM/dQ, dM/dR (1 - nu) / 2
};

// (coordinates and u of the element's corners in cyclic order starting anywhere: all of it is cyclic sums)
__device__ inline StressState stress_state(const double2 (&c)[3], const double2 (&u)[3], double nu)
{
    const double b0 = c[1].y - c[2].y, b1 = c[2].y - c[0].y, b2 = c[0].y - c[1].y;
    const double g0 = c[2].x - c[1].x, g1 = c[0].x - c[2].x, g2 = c[1].x - c[0].x;
    StressState s;
    s.pu = b0 * u[0].x + b1 * u[1].x + b2 * u[2].x;
    s.qu = g0 * u[0].y + g1 * u[1].y + g2 * u[2].y;
    s.ru = (g0 * u[0].x + b0 * u[0].y) + (g1 * u[1].x + b1 * u[1].y) + (g2 * u[2].x + b2 * u[2].y);
    s.A2 = c[0].x * b0 + c[1].x * b1 + c[2].x * b2;
    s.P = s.pu + nu * s.qu;
    s.Q = nu * s.pu + s.qu;
    s.R = 0.5 * (1.0 - nu) * s.ru;
    s.M = (s.P * s.P - s.P * s.Q + s.Q * s.Q) + 3.0 * s.R * s.R;
    s.mP = 2.0 * s.P - s.Q;
    s.mQ = 2.0 * s.Q - s.P;
    s.mR = 3.0 * (1.0 - nu) * s.R;
    return s;
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

struct Member {
    const double2 *xy, *u;
    double youngs, nu;
};

__device__ inline Member member_of(const ObjectiveBatch &ob, int64_t v, int64_t N)
{
    Member m;
    m.xy = (const double2 *)ob.xy + v * (ob.xy_stride / 2);
    m.u = (const double2 *)ob.u + v * N;
    m.youngs = ob.mat[ob.mat_stride * v];
    m.nu = ob.mat[ob.mat_stride * v + 1];
    return m;
}

} // namespace

// ---- 1. per element: terms[e] = w_e (vm_e / scale)^ex, helem[e] = w_e (vm_e / scale)^(ex - 2), nuterm[e] = h_e d(vm_e^2)/dnu
__global__ void __launch_bounds__(256) k_obj_elements(const int32_t *conn, int64_t N, int64_t E, ObjectiveBatch ob)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (e >= E) return;
    const Member m = member_of(ob, v, N);
    double2 c[3], d[3];
    load_corners(m.xy, m.u, conn, e, 0, c, d);
    const StressState s = stress_state(c, d, m.nu);
    const double om = 1.0 - m.nu * m.nu, ci = m.youngs / om / s.A2, k2 = ci * ci;
    const double vm = sqrt(k2 * s.M);
    double h = 0.0, term = 0.0, nut = 0.0;
    if (vm > 0.0) {
        const double r = vm / ob.scale, w = ob.w ? ob.w[v * ob.w_stride + e] : 1.0;
        h = w * pow(r, ob.p - 2.0);
        term = h * (r * r);
        // d/dnu of cs^2 M: dP = q_u, dQ = p_u, dR = -r_u / 2; d(cs^2) = cs^2 4 nu / om
        const double dM = (s.mP * s.qu + s.mQ * s.pu) - 3.0 * s.R * s.ru;
        nut = h * (k2 * (dM + 4.0 * m.nu * s.M / om));
    }
    ob.helem[v * E + e] = h;
    ob.terms[v * E + e] = term;
    ob.nuterm[v * E + e] = nut;
}

// ---- ... least squares, per DOF: g[i] = 2 w_i (u_i - target_i), terms[i] = w_i (u_i - target_i)^2, pxy[i] = 0
__global__ void __launch_bounds__(256) k_obj_lsq(int64_t N, ObjectiveBatch ob)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y, at = v * 2 * N + i;
    if (i >= 2 * N) return;
    const double w = ob.w[v * ob.w_stride + i], d = ob.u[at] - (ob.target ? ob.target[v * ob.target_stride + i] : 0.0);
    const double wd = w * d;
    ob.g[at] = 2.0 * wd;
    ob.terms[at] = wd * d;
    ob.pxy[at] = 0.0;
}

// ---- 2. scalars, stage one: kSensBlocks workgroups per member, each over a fixed share of the n summands
__global__ void __launch_bounds__(256) k_obj_partials(int64_t n, bool with_nu, ObjectiveBatch ob)
{
    __shared__ double s_red[8];
    const int64_t v = blockIdx.y, first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)kSensBlocks * 256;
    const double *terms = ob.terms + v * n, *nuterm = ob.nuterm + v * n;
    double acc[2] = {0.0, 0.0}; // S, the sum of the nu terms
    for (int64_t e = first; e < n; e += step) {
        acc[0] += terms[e];
        if (with_nu) acc[1] += nuterm[e];
    }
    block_sum256<2>(acc, s_red);
    if (threadIdx.x == 0) {
        double *out = ob.partials + 2 * ((int64_t)kSensBlocks * v + blockIdx.x);
        out[0] = acc[0];
        out[1] = acc[1];
    }
}

// ---- ... stage two: one workgroup per member over its kSensBlocks partial records; J, the explicit scalars and the p-norm's
// factor F, which the node kernel reads from here
__global__ void __launch_bounds__(256) k_obj_scalars(ObjectiveBatch ob)
{
    static_assert(kSensBlocks == 256, "one partial record per thread");
    __shared__ double s_red[8];
    const int64_t v = blockIdx.y;
    const double *in = ob.partials + 2 * ((int64_t)kSensBlocks * v + threadIdx.x);
    double acc[2] = {in[0], in[1]};
    block_sum256<2>(acc, s_red);
    if (threadIdx.x != 0) return;
    double *out = ob.scalars + 8 * v;
    const double S = acc[0];
    out[1] = out[2] = out[3] = out[4] = out[5] = out[6] = out[7] = 0.0;
    if (ob.kind == 0) { // MAG_OBJ_DISP_LSQ
        out[0] = S;
        ob.factor[v] = 0.0;
        return;
    }
    double J = 0.0, F = 0.0;
    if (S > 0.0) {
        const double root = pow(S, 1.0 / ob.p);
        J = ob.scale * root;
        F = root / S / (2.0 * ob.scale);
    }
    out[0] = J;
    out[1] = J / ob.mat[ob.mat_stride * v];
    out[2] = F * acc[1];
    ob.factor[v] = F;
}

// One corner's share of a node's sums: h k2 times the derivatives of M / A2^2 of the triangle (c, d: coordinates and
// displacements of its corners in cyclic order, corner 0 the node) with respect to the node's ux, uy (gx, gy) and, u held
// fixed, its x, y (px, py).  cs = E / (1 - nu^2), h = helem of the triangle.
__device__ inline void corner_stress(const double2 (&c)[3], const double2 (&d)[3], double nu, double cs, double h, double &gx,
                                     double &gy, double &px, double &py)
{
    const StressState s = stress_state(c, d, nu);
    const double ia = 1.0 / s.A2, ci = cs * ia, hk = h * (ci * ci);
    const double b0 = c[1].y - c[2].y, g0 = c[2].x - c[1].x;
    const double ax = s.mP + nu * s.mQ, ay = nu * s.mP + s.mQ; // dM/dp_u, dM/dq_u; dM/dr_u = mR
    gx += hk * (ax * b0 + s.mR * g0);
    gy += hk * (ay * g0 + s.mR * b0);
    // x0 enters g1 (+) and g2 (-): dq = uy1 - uy2, dr = ux1 - ux2; y0 enters b1 (-) and b2 (+): dp = ux2 - ux1, dr = uy2 - uy1
    const double dMx = ay * (d[1].y - d[2].y) + s.mR * (d[1].x - d[2].x);
    const double dMy = ax * (d[2].x - d[1].x) + s.mR * (d[2].y - d[1].y);
    px += hk * (dMx - 2.0 * s.M * b0 * ia);
    py += hk * (dMy - 2.0 * s.M * g0 * ia);
}

// ---- 3. per node: g[2i + d] = F sum over the node's incident triangles, in the order of its incidence list, of h_e d(vm_e^2)/du,
// pxy[2i + d] likewise with respect to coordinate d of the node at fixed u.  One workgroup per tile of the Hilbert order and member,
// as k_sens_nodes_tile: the tile's image -- coordinates and u of its owned and halo nodes, each fetched once through perm -- is
// staged in LDS (32 * cap bytes, under 64 KiB at cap = kMaxLdsNodes), the triangles' corners come from the tile-local table, and
// the triangle's h from its id: word k of the node at Hilbert position i is triangle inc[inc_off[i] + k] / 3 (fill_ell16).
__global__ void __launch_bounds__(256) k_obj_nodes_tile(const uint32_t *perm, const int32_t *halo_g, const int32_t *tile_hoff,
                                                         const int32_t *tile_deg, const int64_t *tile_off, const uint32_t *tab,
                                                         const int32_t *inc_off, const uint32_t *inc, int64_t N, int64_t E, int32_t B,
                                                         int32_t cap, ObjectiveBatch ob)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    double2 *s_xy = s_img, *s_u = s_img + cap; // [cap] each: owned nodes 0 .. B-1, halo nodes from B
    const int32_t t = blockIdx.x;
    const int64_t v = blockIdx.y, base = (int64_t)t * B;
    const Member m = member_of(ob, v, N);
    const int32_t hoff = tile_hoff[t], nh = tile_hoff[t + 1] - hoff; // B + nh <= cap
    for (int32_t l = threadIdx.x; l < B; l += 256)
        if (base + l < N) {
            const uint32_t id = perm[base + l];
            s_xy[l] = m.xy[id];
            s_u[l] = m.u[id];
        }
    for (int32_t h = threadIdx.x; h < nh; h += 256) {
        const uint32_t id = perm[halo_g[hoff + h]];
        s_xy[B + h] = m.xy[id];
        s_u[B + h] = m.u[id];
    }
    __syncthreads();
    const double cs = m.youngs / (1.0 - m.nu * m.nu), F = ob.factor[v];
    const double *helem = ob.helem + v * E;
    const int32_t td = tile_deg[t];
    const uint32_t *table = tab + tile_off[t];
    for (int32_t l = threadIdx.x; l < B; l += 256) {
        if (base + l >= N) break;
        double2 c[3], d[3];
        c[0] = s_xy[l];
        d[0] = s_u[l];
        const uint32_t *tris = inc + inc_off[base + l];
        double gx = 0.0, gy = 0.0, px = 0.0, py = 0.0;
        for (int32_t k = 0; k < td; ++k) {
            const uint32_t w = table[(int64_t)k * B + l];
            if (w == 0xffffffffu) break; // (a node's words are its list's, in order, then the filler)
            const uint32_t lb = w & 0xffffu, lc = w >> 16;
            c[1] = s_xy[lb];
            c[2] = s_xy[lc];
            d[1] = s_u[lb];
            d[2] = s_u[lc];
            corner_stress(c, d, m.nu, cs, helem[tris[k] / 3u], gx, gy, px, py);
        }
        const int64_t at = v * N + perm[base + l];
        ((double2 *)ob.g)[at] = make_double2(F * gx, F * gy);
        ((double2 *)ob.pxy)[at] = make_double2(F * px, F * py);
    }
}

// ---- ... the same sums gathered from memory (a tile image too large for the LDS, or MAG_TUNE_SENS_STAGE=0): lane g takes node
// perm[g], inc[k] = 3e + (corner of e that is this node), ascending per node.  The same arithmetic in the same order: the same bits.
__global__ void __launch_bounds__(256) k_obj_nodes(const int32_t *inc_off, const uint32_t *inc, const uint32_t *perm,
                                                    const int32_t *conn, int64_t N, int64_t E, ObjectiveBatch ob)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (g >= N) return;
    const Member m = member_of(ob, v, N);
    const double cs = m.youngs / (1.0 - m.nu * m.nu), F = ob.factor[v];
    const double *helem = ob.helem + v * E;
    double gx = 0.0, gy = 0.0, px = 0.0, py = 0.0;
    const int32_t k1 = inc_off[g + 1];
    for (int32_t k = inc_off[g]; k < k1; ++k) {
        const uint32_t w = inc[k];
        const int64_t e = w / 3u;
        double2 c[3], d[3];
        load_corners(m.xy, m.u, conn, e, (int)(w - 3u * (uint32_t)e), c, d); // corner 0 is this node
        corner_stress(c, d, m.nu, cs, helem[e], gx, gy, px, py);
    }
    const int64_t at = v * N + perm[g];
    ((double2 *)ob.g)[at] = make_double2(F * gx, F * gy);
    ((double2 *)ob.pxy)[at] = make_double2(F * px, F * py);
}

// ---- 4. totals: explicit + adjoint, one add per entry
__global__ void __launch_bounds__(256) k_obj_totals(int64_t N, const double *pxy, const double *adj_dxy, const double *adj_scalars,
                                                     double *dxy, double *scalars)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y, at = v * 2 * N + i;
    if (i < 2 * N) dxy[at] = pxy[at] + adj_dxy[at];
    if (i < 3) scalars[8 * v + 4 + i] = scalars[8 * v + 1 + i] + adj_scalars[8 * v + 1 + i];
    if (i == 3) scalars[8 * v + 7] = 1.0;
}

void objective(const SensMesh &m, const ObjectiveBatch &ob, hipStream_t s)
{
    const unsigned n = (unsigned)ob.count;
    const int64_t N = m.N, E = m.E;
    if (ob.kind == 0) { // MAG_OBJ_DISP_LSQ
        k_obj_lsq<<<dim3((unsigned)((2 * N + 255) / 256), n), 256, 0, s>>>(N, ob);
        k_obj_partials<<<dim3(kSensBlocks, n), 256, 0, s>>>(2 * N, false, ob);
        k_obj_scalars<<<dim3(1, n), 256, 0, s>>>(ob);
        return;
    }
    k_obj_elements<<<dim3((unsigned)((E + 255) / 256), n), 256, 0, s>>>(m.conn, N, E, ob);
    k_obj_partials<<<dim3(kSensBlocks, n), 256, 0, s>>>(E, true, ob);
    k_obj_scalars<<<dim3(1, n), 256, 0, s>>>(ob);
    if (m.tab)
        k_obj_nodes_tile<<<dim3((unsigned)m.T, n), 256, 32 * (size_t)m.cap, s>>>(m.perm, m.halo_g, m.tile_hoff, m.tile_deg, m.tile_off,
                                                                                 m.tab, m.inc_off, m.inc, N, E, m.B, m.cap, ob);
    else
        k_obj_nodes<<<dim3((unsigned)((N + 255) / 256), n), 256, 0, s>>>(m.inc_off, m.inc, m.perm, m.conn, N, E, ob);
}

void objective_totals(int64_t N, int32_t count, const double *pxy, const double *adj_dxy, const double *adj_scalars, double *dxy,
                      double *scalars, hipStream_t s)
{
    k_obj_totals<<<dim3((unsigned)((2 * N + 255) / 256), (unsigned)count), 256, 0, s>>>(N, pxy, adj_dxy, adj_scalars, dxy, scalars);
}

} // namespace magk
