// The bilinear pass of mag_run_adjoint: for solved members with displacements u and adjoint solutions lambda, the derivatives
// dJ/dtheta = -lambda^T (dK/dtheta) u with respect to an element-wise stiffness scale, every node coordinate, E, nu and the
// thickness, and dJ/d(loads), on the skeleton of member_pass.h: one pass over elements, one over nodes, one over DOFs, a
// two-stage reduction -- per member, the member from blockIdx.y.  Compiled -ffp-contract=off: the rounding is the source's.
//
// With p_v, q_v, r_v of v = u and v = l (lambda) and A2 as in member_pass.h and
//   Qb = p_l p_u + q_l q_u + nu (p_l q_u + q_l p_u) + (1 - nu) / 2 r_l r_u,       A2 = 2A,  om = 1 - nu^2,
// the element's bilinear form is l_e^T K_e u_e = E t Qb / (2 A2 om) (Qb = Q of sens.hip where l = u: twice the energy); its
// derivatives follow in closed form as there.
#include "adjoint.h"
#include "member_pass.h"

namespace magk {

namespace {

struct BilinearState {
    double pu, qu, ru, pl, ql, rl, A2, b0, g0;
};

// (coordinates, u and lambda of the element's corners in cyclic order starting anywhere)
__device__ inline BilinearState bilinear_state(const double2 (&c)[3], const double2 (&u)[3], const double2 (&l)[3])
{
    const Edges e = edges_of(c);
    const Sums su = cyclic_sums(e, u), sl = cyclic_sums(e, l);
    return {su.p, su.q, su.r, sl.p, sl.q, sl.r, e.A2, e.b[0], e.g[0]};
}

__device__ inline double bilinear_Q(const BilinearState &s, double nu)
{
    return s.pl * s.pu + s.ql * s.qu + nu * (s.pl * s.qu + s.ql * s.pu) + 0.5 * (1.0 - nu) * s.rl * s.ru;
}

// One corner's share of a node's sum: the derivative of l_e^T K_e u_e of the triangle (c, d, l: coordinates, u and lambda of its
// corners in cyclic order, corner 0 the node) with respect to the node's x and y, u and lambda held fixed.  cm = E t / (2 om).
__device__ inline void corner_bilinear(const double2 (&c)[3], const double2 (&d)[3], const double2 (&l)[3], double nu, double cm,
                                       double &gx, double &gy)
{
    const BilinearState s = bilinear_state(c, d, l);
    const double Qb = bilinear_Q(s, nu), ia = 1.0 / s.A2, h = 0.5 * (1.0 - nu);
    // x0 enters g1 (+) and g2 (-): dq_v = vy1 - vy2, dr_v = vx1 - vx2; y0 enters b1 (-) and b2 (+): dp_v = vx2 - vx1, dr_v = vy2 - vy1
    const double dQx = (s.ql + nu * s.pl) * (d[1].y - d[2].y) + (s.qu + nu * s.pu) * (l[1].y - l[2].y) +
                       h * ((l[1].x - l[2].x) * s.ru + s.rl * (d[1].x - d[2].x));
    const double dQy = (s.pl + nu * s.ql) * (d[2].x - d[1].x) + (s.pu + nu * s.qu) * (l[2].x - l[1].x) +
                       h * ((l[2].y - l[1].y) * s.ru + s.rl * (d[2].y - d[1].y));
    gx += cm * ia * (dQx - Qb * s.b0 * ia);
    gy += cm * ia * (dQy - Qb * s.g0 * ia);
}

__device__ inline const double2 *lambda_of(const AdjointBatch &ab, int64_t v, int64_t N) { return (const double2 *)ab.lam + v * N; }

// The node pass: dxy[2i + d] = -(sum over the node's incident triangles, in the order of its incidence list, of the derivative
// of l_e^T K_e u_e with respect to coordinate d of the node).  Fields: coordinates, u, lambda.
struct Bilinear : ScaledCorners {
    double nu, cm;
    double2 *dxy;
    __device__ Bilinear(const Member &m, const AdjointBatch &ab, const SensMesh &mesh)
        : ScaledCorners(m, mesh), nu(m.nu), cm(m.youngs * m.thick / (2.0 * (1.0 - m.nu * m.nu))), dxy((double2 *)ab.dxy)
    {
    }
    __device__ void corner(Node &n, const double2 (&f)[3][3], int32_t k) const
    {
        corner_bilinear(f[0], f[1], f[2], nu, factor(n, k, cm), n.gx, n.gy);
    }
    __device__ void store(const Node &n, int64_t at) const { dxy[at] = make_double2(-n.gx, -n.gy); }
};

} // namespace

// ---- 1. per element: delem[e] = -l_e^T K_e u_e and l_e^T (dK_e / dnu) u_e
__global__ void __launch_bounds__(256) k_adjoint_elements(const int32_t *conn, int64_t N, int64_t E, AdjointBatch ab)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (e >= E) return;
    const Member m = member_of(ab, v, N);
    const double2 *const src[3] = {m.xy, m.u, lambda_of(ab, v, N)};
    double2 f[3][3];
    load_corners(src, conn, e, 0, f);
    const BilinearState s = bilinear_state(f[0], f[1], f[2]);
    const double Qb = bilinear_Q(s, m.nu), om = 1.0 - m.nu * m.nu;
    double k = m.youngs * m.thick / (2.0 * s.A2);
    if (m.scale) k *= m.scale[e];
    ab.delem[v * E + e] = -(k * Qb / om);
    // d/dnu of Qb / (1 - nu^2)
    ab.nuterm[v * E + e] = k * (((s.pl * s.qu + s.ql * s.pu) - 0.5 * s.rl * s.ru) / om + 2.0 * m.nu * Qb / (om * om));
}

// ---- 2. per node, on the tile's image in LDS: 48 * cap bytes, up to 96768 at cap = kMaxLdsNodes (one workgroup per CU then, one
// wave per SIMD; the launch wrapper raises the 64 KiB default limit) ...
__global__ void __launch_bounds__(256) k_adjoint_nodes_tile(SensMesh mesh, AdjointBatch ab)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    const Member m = member_of(ab, blockIdx.y, mesh.N);
    const double2 *const src[3] = {m.xy, m.u, lambda_of(ab, blockIdx.y, mesh.N)};
    tile_walk(mesh, src, s_img, Bilinear(m, ab, mesh));
}

// ---- ... or gathered from memory
__global__ void __launch_bounds__(256) k_adjoint_nodes(SensMesh mesh, AdjointBatch ab)
{
    const Member m = member_of(ab, blockIdx.y, mesh.N);
    const double2 *const src[3] = {m.xy, m.u, lambda_of(ab, blockIdx.y, mesh.N)};
    gather_walk(mesh, src, Bilinear(m, ab, mesh));
}

// ---- 3. per DOF: dJ/df_in = lambda on a free DOF, dJ/du_in = g - (K lambda) on a prescribed one
__global__ void __launch_bounds__(256) k_adjoint_dloads(const uint8_t *u_known, int64_t N, AdjointBatch ab)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, at = (int64_t)blockIdx.y * 2 * N + i;
    if (i >= 2 * N) return;
    ab.dloads[at] = u_known[i] ? ab.g[at] - ab.f_adj[at] : ab.lam[at];
}

// ---- 4. scalars, stage one: the sum of delem, the sum of the nu terms over the elements
__global__ void __launch_bounds__(256) k_adjoint_partials(int64_t E, AdjointBatch ab)
{
    const double *delem = ab.delem + blockIdx.y * E, *nuterm = ab.nuterm + blockIdx.y * E;
    double acc[2] = {0.0, 0.0};
    share_sum(E, acc, [=](int64_t e, double (&a)[2]) {
        a[0] += delem[e];
        a[1] += nuterm[e];
    });
    store_partials(acc, ab.partials);
}

// ---- ... stage two
__global__ void __launch_bounds__(256) k_adjoint_scalars(AdjointBatch ab)
{
    sum_partials<2>(ab.partials, [&](int64_t v, const double (&acc)[2]) {
        double *out = ab.scalars + 8 * v;
        out[0] = -acc[0]; // a = sum of l_e^T K_e u_e
        out[1] = acc[0] / ab.mat[ab.mat_stride * v];
        out[2] = -acc[1];
        out[3] = acc[0] / ab.mat[ab.mat_stride * v + 2];
        out[4] = out[5] = out[6] = out[7] = 0.0;
    });
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
        k_adjoint_nodes_tile<<<dim3((unsigned)m.T, n), 256, lds, s>>>(m, ab);
    } else {
        k_adjoint_nodes<<<dim3((unsigned)((N + 255) / 256), n), 256, 0, s>>>(m, ab);
    }
    k_adjoint_dloads<<<dim3((unsigned)((2 * N + 255) / 256), n), 256, 0, s>>>(m.u_known, N, ab);
    k_adjoint_partials<<<dim3(kSensBlocks, n), 256, 0, s>>>(E, ab);
    k_adjoint_scalars<<<dim3(1, n), 256, 0, s>>>(ab);
    return hipSuccess;
}

} // namespace magk
