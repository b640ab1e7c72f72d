// Energy and design sensitivities of solved members (mag_run_sensitivities): strain energy per element, its gradient with
// respect to every node coordinate, and the scalar objective terms, on the skeleton of member_pass.h: one pass over elements,
// one over nodes, a two-stage reduction -- per member, the member taken from blockIdx.y as the _v kernels of exact.hip do.
// Everything is in the caller's numbering.  Compiled -ffp-contract=off: the rounding is the source's.
//
// With p, q, r of u and A2 as in member_pass.h and
//   Q = p^2 + q^2 + 2 nu p q + (1 - nu) / 2 r^2,
// the element's energy is 1/2 u_e^T K_e u_e = E t Q / (4 A2 (1 - nu^2)); its derivatives follow in closed form.
#include "member_pass.h"

namespace magk {

namespace {

struct ElemState {
    double p, q, r, A2, b0, g0;
};

// (x, y, ux, uy of the element's corners in cyclic order starting anywhere)
__device__ inline ElemState elem_state(const double2 (&c)[3], const double2 (&u)[3])
{
    const Edges e = edges_of(c);
    const Sums s = cyclic_sums(e, u);
    return {s.p, s.q, s.r, e.A2, e.b[0], e.g[0]};
}

__device__ inline double elem_Q(const ElemState &s, double nu)
{
    return s.p * s.p + s.q * s.q + 2.0 * nu * s.p * s.q + 0.5 * (1.0 - nu) * s.r * s.r;
}

// One corner's share of a node's gradient: the derivative of the energy of the triangle (c, d: coordinates and displacements
// of its corners in cyclic order, corner 0 the node) with respect to the node's x and y, u held fixed.
__device__ inline void corner_gradient(const double2 (&c)[3], const double2 (&d)[3], double nu, double cm, double &gx, double &gy)
{
    const ElemState s = elem_state(c, d);
    const double Q = elem_Q(s, nu), ia = 1.0 / s.A2;
    // x0 enters g1 (+) and g2 (-): dq = uy1 - uy2, dr = ux1 - ux2; y0 enters b1 (-) and b2 (+): dp = ux2 - ux1, dr = uy2 - uy1
    const double dQx = 2.0 * (s.q + nu * s.p) * (d[1].y - d[2].y) + (1.0 - nu) * s.r * (d[1].x - d[2].x);
    const double dQy = 2.0 * (s.p + nu * s.q) * (d[2].x - d[1].x) + (1.0 - nu) * s.r * (d[2].y - d[1].y);
    gx += cm * ia * (dQx - Q * s.b0 * ia);
    gy += cm * ia * (dQy - Q * s.g0 * ia);
}

// The node pass: dxy[2i + d] = sum over the node's incident triangles, in the order of its incidence list, of the triangle's
// energy derivative with respect to coordinate d of the node (u held fixed).  Fields: coordinates, u.
struct Gradient : ScaledCorners {
    double nu, cm;
    double2 *dxy;
    __device__ Gradient(const Member &m, const SensBatch &sb, const SensMesh &mesh)
        : ScaledCorners(m, mesh), nu(m.nu), cm(m.youngs * m.thick / (4.0 * (1.0 - m.nu * m.nu))), dxy((double2 *)sb.dxy)
    {
    }
    __device__ void corner(Node &n, const double2 (&f)[2][3], int32_t k) const
    {
        corner_gradient(f[0], f[1], nu, factor(n, k, cm), n.gx, n.gy);
    }
    __device__ void store(const Node &n, int64_t at) const { dxy[at] = make_double2(n.gx, n.gy); }
};

} // namespace

// ---- 1. per element: energy[e] = 1/2 u_e^T K_e u_e and d(energy[e]) / d(nu)
__global__ void __launch_bounds__(256) k_sens_energy(const int32_t *conn, int64_t N, int64_t E, SensBatch sb)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (e >= E) return;
    const Member m = member_of(sb, v, N);
    const double2 *const src[2] = {m.xy, m.u};
    double2 f[2][3];
    load_corners(src, conn, e, 0, f);
    const ElemState s = elem_state(f[0], f[1]);
    const double Q = elem_Q(s, m.nu), om = 1.0 - m.nu * m.nu;
    double k = m.youngs * m.thick / (4.0 * s.A2);
    if (m.scale) k *= m.scale[e];
    sb.energy[v * E + e] = k * Q / om;
    // d/dnu of Q / (1 - nu^2)
    sb.nuterm[v * E + e] = k * ((2.0 * s.p * s.q - 0.5 * s.r * s.r) / om + 2.0 * m.nu * Q / (om * om));
}

// ---- 2. per node, on the tile's image in LDS (32 * cap bytes) ...
__global__ void __launch_bounds__(256) k_sens_nodes_tile(SensMesh mesh, SensBatch sb)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    const Member m = member_of(sb, blockIdx.y, mesh.N);
    const double2 *const src[2] = {m.xy, m.u};
    tile_walk(mesh, src, s_img, Gradient(m, sb, mesh));
}

// ---- ... or gathered from memory
__global__ void __launch_bounds__(256) k_sens_nodes(SensMesh mesh, SensBatch sb)
{
    const Member m = member_of(sb, blockIdx.y, mesh.N);
    const double2 *const src[2] = {m.xy, m.u};
    gather_walk(mesh, src, Gradient(m, sb, mesh));
}

// ---- 3. scalars, stage one: W, dW/dnu over the elements; external work, reaction work over the DOFs
__global__ void __launch_bounds__(256) k_sens_partials(const uint8_t *u_known, int64_t N, int64_t E, SensBatch sb)
{
    const int64_t v = blockIdx.y;
    const double *energy = sb.energy + v * E, *nuterm = sb.nuterm + v * E;
    const double *u = sb.u + v * 2 * N, *f = sb.f_out + v * 2 * N;
    const double *u_in = sb.u_in + v * sb.loads_stride, *f_in = sb.f_in + v * sb.loads_stride;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    share_sum(E, acc, [=](int64_t e, double (&a)[4]) {
        a[0] += energy[e];
        a[1] += nuterm[e];
    });
    share_sum(2 * N, acc, [=](int64_t i, double (&a)[4]) {
        if (u_known[i])
            a[3] += f[i] * u_in[i];
        else
            a[2] += f_in[i] * u[i];
    });
    store_partials(acc, sb.partials);
}

// ---- ... stage two
__global__ void __launch_bounds__(256) k_sens_scalars(SensBatch sb)
{
    sum_partials<4>(sb.partials, [&](int64_t v, const double (&acc)[4]) {
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
    });
}

void sensitivities(const SensMesh &m, const SensBatch &sb, hipStream_t s)
{
    const unsigned n = (unsigned)sb.count;
    const int64_t N = m.N, E = m.E;
    k_sens_energy<<<dim3((unsigned)((E + 255) / 256), n), 256, 0, s>>>(m.conn, N, E, sb);
    if (m.tab)
        k_sens_nodes_tile<<<dim3((unsigned)m.T, n), 256, 32 * (size_t)m.cap, s>>>(m, sb);
    else
        k_sens_nodes<<<dim3((unsigned)((N + 255) / 256), n), 256, 0, s>>>(m, sb);
    k_sens_partials<<<dim3(kSensBlocks, n), 256, 0, s>>>(m.u_known, N, E, sb);
    k_sens_scalars<<<dim3(1, n), 256, 0, s>>>(sb);
}

} // namespace magk
