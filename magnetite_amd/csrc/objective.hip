// Objectives of solved members on the device (mag_run_objective): J, g = dJ/du and J's explicit partials at fixed u -- what the
// adjoint pass (mag_run_adjoint) takes and what the caller would otherwise add to its results --, on the skeleton of
// member_pass.h: one pass over elements, the two-stage reduction, one pass over nodes -- per member, the member from blockIdx.y.
// Compiled -ffp-contract=off: the rounding is the source's.
//
// MAG_OBJ_STRESS_PNORM.  sigma_e = D B u_e with the reference's D, B and SIGNED area (d_element_stress, exact.hip).  In the
// notation of member_pass.h, p_u, q_u, r_u the cyclic sums of u, A2 = 2A, and with
//   P = p_u + nu q_u,  Q = nu p_u + q_u,  R = (1 - nu) / 2 r_u,  cs = E / (1 - nu^2):   (sx, sy, txy) = cs / A2 (P, Q, R),
//   M = P^2 - P Q + Q^2 + 3 R^2,      vm_e^2 = (cs / A2)^2 M.
// S = sum_e w_e (vm_e / scale)^ex, J = scale S^(1/ex).  With h_e = w_e (vm_e / scale)^(ex - 2) and F = S^(1/ex - 1) / (2 scale),
//   dJ/dz = F sum_e h_e d(vm_e^2)/dz                      for z = a displacement, a coordinate (u fixed), nu (u fixed),
// and d(vm_e^2)/dz follows in closed form from mP = dM/dP = 2P - Q, mQ = dM/dQ = 2Q - P, mR = dM/dR (1 - nu) / 2 = 3 (1 - nu) R.
// An element with vm_e = 0 has h_e = 0: it contributes nothing to S, g or the partials.
//
// MAG_OBJ_DISP_LSQ.  J = sum_i w_i (u_i - target_i)^2, g = 2 w (u - target); no explicit partial.
#include "objective.h"
#include "member_pass.h"

namespace magk {

namespace {

struct StressState {
    double pu, qu, ru, A2, b0, g0; // p, q, r of u, 2A, the node's two edge differences
    double P, Q, R, M;             // as above
    double mP, mQ, mR;             // dM/dP, dM/dQ, dM/dR (1 - nu) / 2
};

// (coordinates and u of the element's corners in cyclic order starting anywhere)
__device__ inline StressState stress_state(const double2 (&c)[3], const double2 (&u)[3], double nu)
{
    const Edges e = edges_of(c);
    const Sums su = cyclic_sums(e, u);
    StressState s;
    s.pu = su.p, s.qu = su.q, s.ru = su.r, s.A2 = e.A2, s.b0 = e.b[0], s.g0 = e.g[0];
    s.P = s.pu + nu * s.qu;
    s.Q = nu * s.pu + s.qu;
    s.R = 0.5 * (1.0 - nu) * s.ru;
    s.M = (s.P * s.P - s.P * s.Q + s.Q * s.Q) + 3.0 * s.R * s.R;
    s.mP = 2.0 * s.P - s.Q;
    s.mQ = 2.0 * s.Q - s.P;
    s.mR = 3.0 * (1.0 - nu) * s.R;
    return s;
}

// One corner's share of a node's sums: h k2 times the derivatives of M / A2^2 of the triangle (c, d: coordinates and
// displacements of its corners in cyclic order, corner 0 the node) with respect to the node's ux, uy (gx, gy) and, u held
// fixed, its x, y (px, py).  cs = E / (1 - nu^2), h = helem of the triangle.
__device__ inline void corner_stress(const double2 (&c)[3], const double2 (&d)[3], double nu, double cs, double h, double &gx,
                                     double &gy, double &px, double &py)
{
    const StressState s = stress_state(c, d, nu);
    const double ia = 1.0 / s.A2, ci = cs * ia, hk = h * (ci * ci);
    const double ax = s.mP + nu * s.mQ, ay = nu * s.mP + s.mQ; // dM/dp_u, dM/dq_u; dM/dr_u = mR
    gx += hk * (ax * s.b0 + s.mR * s.g0);
    gy += hk * (ay * s.g0 + s.mR * s.b0);
    // x0 enters g1 (+) and g2 (-): dq = uy1 - uy2, dr = ux1 - ux2; y0 enters b1 (-) and b2 (+): dp = ux2 - ux1, dr = uy2 - uy1
    const double dMx = ay * (d[1].y - d[2].y) + s.mR * (d[1].x - d[2].x);
    const double dMy = ax * (d[2].x - d[1].x) + s.mR * (d[2].y - d[1].y);
    px += hk * (dMx - 2.0 * s.M * s.b0 * ia);
    py += hk * (dMy - 2.0 * s.M * s.g0 * ia);
}

// The node pass: g[2i + d] = F sum over the node's incident triangles, in the order of its incidence list, of h_e d(vm_e^2)/du,
// pxy[2i + d] likewise with respect to coordinate d of the node at fixed u.  Fields: coordinates, u.  The triangle's h comes
// from its id, which the node's incidence list gives (as fill_ell16 laid the tile-local table's words out).
struct Stress {
    double nu, cs, F;
    const double *helem;
    const int32_t *inc_off;
    const uint32_t *inc;
    double2 *g, *pxy;
    struct Node {
        const uint32_t *tris;
        double gx, gy, px, py;
    };
    __device__ Stress(const SensMesh &mesh, const Member &m, const ObjectiveBatch &ob, int64_t v)
        : nu(m.nu), cs(m.youngs / (1.0 - m.nu * m.nu)), F(ob.factor[v]), helem(ob.helem + v * mesh.E), inc_off(mesh.inc_off),
          inc(mesh.inc), g((double2 *)ob.g), pxy((double2 *)ob.pxy)
    {
    }
    __device__ Node node(int64_t pos) const { return {inc + inc_off[pos], 0.0, 0.0, 0.0, 0.0}; }
    __device__ void corner(Node &n, const double2 (&f)[2][3], int32_t k) const
    {
        corner_stress(f[0], f[1], nu, cs, helem[n.tris[k] / 3u], n.gx, n.gy, n.px, n.py);
    }
    __device__ void store(const Node &n, int64_t at) const
    {
        g[at] = make_double2(F * n.gx, F * n.gy);
        pxy[at] = make_double2(F * n.px, F * n.py);
    }
};

} // namespace

// ---- 1. per element: terms[e] = w_e (vm_e / scale)^ex, helem[e] = w_e (vm_e / scale)^(ex - 2), nuterm[e] = h_e d(vm_e^2)/dnu
__global__ void __launch_bounds__(256) k_obj_elements(const int32_t *conn, int64_t N, int64_t E, ObjectiveBatch ob)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (e >= E) return;
    const Member m = member_of(ob, v, N);
    const double2 *const src[2] = {m.xy, m.u};
    double2 f[2][3];
    load_corners(src, conn, e, 0, f);
    const StressState s = stress_state(f[0], f[1], m.nu);
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

// ---- 2. scalars, stage one: S and the sum of the nu terms over the n summands
__global__ void __launch_bounds__(256) k_obj_partials(int64_t n, bool with_nu, ObjectiveBatch ob)
{
    const double *terms = ob.terms + blockIdx.y * n, *nuterm = ob.nuterm + blockIdx.y * n;
    double acc[2] = {0.0, 0.0};
    share_sum(n, acc, [=](int64_t e, double (&a)[2]) {
        a[0] += terms[e];
        if (with_nu) a[1] += nuterm[e];
    });
    store_partials(acc, ob.partials);
}

// ---- ... stage two: J, the explicit scalars and the p-norm's factor F, which the node kernel reads from here
__global__ void __launch_bounds__(256) k_obj_scalars(ObjectiveBatch ob)
{
    sum_partials<2>(ob.partials, [&](int64_t v, const double (&acc)[2]) {
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
    });
}

// ---- 3. per node, on the tile's image in LDS (32 * cap bytes, under 64 KiB at cap = kMaxLdsNodes) ...
__global__ void __launch_bounds__(256) k_obj_nodes_tile(SensMesh mesh, ObjectiveBatch ob)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    const Member m = member_of(ob, blockIdx.y, mesh.N);
    const double2 *const src[2] = {m.xy, m.u};
    tile_walk(mesh, src, s_img, Stress(mesh, m, ob, blockIdx.y));
}

// ---- ... or gathered from memory
__global__ void __launch_bounds__(256) k_obj_nodes(SensMesh mesh, ObjectiveBatch ob)
{
    const Member m = member_of(ob, blockIdx.y, mesh.N);
    const double2 *const src[2] = {m.xy, m.u};
    gather_walk(mesh, src, Stress(mesh, m, ob, blockIdx.y));
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
        k_obj_nodes_tile<<<dim3((unsigned)m.T, n), 256, 32 * (size_t)m.cap, s>>>(m, ob);
    else
        k_obj_nodes<<<dim3((unsigned)((N + 255) / 256), n), 256, 0, s>>>(m, ob);
}

void objective_totals(int64_t N, int32_t count, const double *pxy, const double *adj_dxy, const double *adj_scalars, double *dxy,
                      double *scalars, hipStream_t s)
{
    k_obj_totals<<<dim3((unsigned)((2 * N + 255) / 256), (unsigned)count), 256, 0, s>>>(N, pxy, adj_dxy, adj_scalars, dxy, scalars);
}

} // namespace magk
