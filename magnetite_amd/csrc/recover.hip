// Stress recovery of solved members (mag_run_stress): the stress tensor and von Mises value per element, the continuous nodal
// field by area-weighted averaging, the Zienkiewicz-Zhu error indicator per element and the scalars, on the skeleton of
// member_pass.h: passes over elements, one over nodes, a two-stage reduction -- per member, the member from blockIdx.y.
// Everything is in the caller's numbering.  Compiled -ffp-contract=off: the rounding is the source's.
//
// sigma_e = D B u_e with the reference's D, B and SIGNED area (d_element_stress, exact.hip; B carries 1 / A2, so the tensor is
// the physical one for either orientation).  In the notation of member_pass.h, p_u, q_u, r_u the cyclic sums of u, A2 = 2A:
//   (sx, sy, txy) = E / ((1 - nu^2) A2) (p_u + nu q_u, nu p_u + q_u, (1 - nu) / 2 r_u),
//   vm = sqrt(sx^2 - sx sy + sy^2 + 3 txy^2)                    (objective.hip's vm_e),
//   sigma*_i = (sum over the triangles e of node i of |A_e| sigma_e) / (sum of |A_e|), in the order of the incidence list,
//   with C = D^-1:  s^T C s = (sx^2 - 2 nu sx sy + sy^2 + 2 (1 + nu) txy^2) / E,   d_k = sigma*_{n_k} - sigma_e,
//   eta2[e] = |A_e| t / 12 (sum_k d_k^T C d_k + (sum_k d_k)^T C (sum_k d_k)),
// the exact integral over the triangle of (sigma* - sigma_e)^T C (sigma* - sigma_e) t with sigma* interpolated linearly.
#include "recover.h"
#include "member_pass.h"

namespace magk {

namespace {

struct Tensor {
    double sx, sy, txy;
};

// (coordinates and u of the element's corners in cyclic order starting anywhere; cs = E / (1 - nu^2))
__device__ inline Tensor tensor_of(const double2 (&c)[3], const double2 (&u)[3], double nu, double cs, double &A2)
{
    const Edges e = edges_of(c);
    const Sums s = cyclic_sums(e, u);
    const double ci = cs / e.A2;
    A2 = e.A2;
    return {ci * (s.p + nu * s.q), ci * (nu * s.p + s.q), ci * (0.5 * (1.0 - nu) * s.r)};
}

__device__ inline double von_mises(const Tensor &t)
{
    return sqrt((t.sx * t.sx - t.sx * t.sy + t.sy * t.sy) + 3.0 * t.txy * t.txy);
}

// E s^T C s
__device__ inline double compliance(const Tensor &t, double nu)
{
    return (t.sx * t.sx - 2.0 * nu * t.sx * t.sy + t.sy * t.sy) + 2.0 * (1.0 + nu) * t.txy * t.txy;
}

// a row of four as two 16-byte stores
__device__ inline void store_row(double *rows, int64_t at, const Tensor &t, double vm)
{
    double2 *out = (double2 *)rows + 2 * at;
    out[0] = make_double2(t.sx, t.sy);
    out[1] = make_double2(t.txy, vm);
}

__device__ inline Tensor load_tensor(const double *rows, int64_t at)
{
    const double2 *in = (const double2 *)rows + 2 * at;
    const double2 a = in[0];
    return {a.x, a.y, in[1].x};
}

// The node pass: the |A|-weighted sums of the tensors of the node's incident triangles, in the order of its incidence list,
// and the sum of the weights; the node's row is their quotient and its von Mises value, four zeros for a node that no
// element touches.  Fields: coordinates, u.
struct Average {
    double nu, cs;
    double *rows;
    struct Node {
        double sx, sy, txy, w;
    };
    __device__ Average(const Member &m, const StressBatch &sb) : nu(m.nu), cs(m.youngs / (1.0 - m.nu * m.nu)), rows(sb.node) {}
    __device__ Node node(int64_t) const { return {0.0, 0.0, 0.0, 0.0}; }
    __device__ void corner(Node &n, const double2 (&f)[2][3], int32_t) const
    {
        double A2;
        const Tensor t = tensor_of(f[0], f[1], nu, cs, A2);
        const double a = 0.5 * fabs(A2);
        n.sx += a * t.sx;
        n.sy += a * t.sy;
        n.txy += a * t.txy;
        n.w += a;
    }
    __device__ void store(const Node &n, int64_t at) const
    {
        Tensor t = {0.0, 0.0, 0.0};
        if (n.w > 0.0) t = {n.sx / n.w, n.sy / n.w, n.txy / n.w};
        store_row(rows, at, t, von_mises(t));
    }
};

} // namespace

// ---- 1. per element: elem[e] = (sx, sy, txy, vm)
__global__ void __launch_bounds__(256) k_rec_elements(const int32_t *conn, int64_t N, int64_t E, StressBatch sb)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (e >= E) return;
    const Member m = member_of(sb, v, N);
    const double2 *const src[2] = {m.xy, m.u};
    double2 f[2][3];
    load_corners(src, conn, e, 0, f);
    double A2;
    const Tensor t = tensor_of(f[0], f[1], m.nu, m.youngs / (1.0 - m.nu * m.nu), A2);
    store_row(sb.elem, v * E + e, t, von_mises(t));
}

// ---- 2. per node, on the tile's image in LDS (32 * cap bytes, under 64 KiB at cap = kMaxLdsNodes) ...
__global__ void __launch_bounds__(256) k_rec_nodes_tile(SensMesh mesh, StressBatch sb)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    const Member m = member_of(sb, blockIdx.y, mesh.N);
    const double2 *const src[2] = {m.xy, m.u};
    tile_walk(mesh, src, s_img, Average(m, sb));
}

// ---- ... or gathered from memory
__global__ void __launch_bounds__(256) k_rec_nodes(SensMesh mesh, StressBatch sb)
{
    const Member m = member_of(sb, blockIdx.y, mesh.N);
    const double2 *const src[2] = {m.xy, m.u};
    gather_walk(mesh, src, Average(m, sb));
}

// ---- 3. per element: eta2[e] from the rows of its three nodes and its own, uterm[e] = |A_e| t sigma_e^T C sigma_e
__global__ void __launch_bounds__(256) k_rec_error(const int32_t *conn, int64_t N, int64_t E, StressBatch sb)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (e >= E) return;
    const Member m = member_of(sb, v, N);
    const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
    const double2 c[3] = {m.xy[n0], m.xy[n1], m.xy[n2]};
    const double at = 0.5 * fabs(edges_of(c).A2) * m.thick / m.youngs; // |A_e| t / E
    const Tensor se = load_tensor(sb.elem, v * E + e);
    const Tensor s0 = load_tensor(sb.node, v * N + n0), s1 = load_tensor(sb.node, v * N + n1), s2 = load_tensor(sb.node, v * N + n2);
    const Tensor d0 = {s0.sx - se.sx, s0.sy - se.sy, s0.txy - se.txy};
    const Tensor d1 = {s1.sx - se.sx, s1.sy - se.sy, s1.txy - se.txy};
    const Tensor d2 = {s2.sx - se.sx, s2.sy - se.sy, s2.txy - se.txy};
    const Tensor ds = {d0.sx + d1.sx + d2.sx, d0.sy + d1.sy + d2.sy, d0.txy + d1.txy + d2.txy};
    const double q = (compliance(d0, m.nu) + compliance(d1, m.nu) + compliance(d2, m.nu)) + compliance(ds, m.nu);
    sb.eta2[v * E + e] = at / 12.0 * q;
    sb.uterm[v * E + e] = at * compliance(se, m.nu);
}

// ---- 4. scalars, stage one: the sums of eta2 and uterm and the largest vm over the elements, the largest vm over the nodes
__global__ void __launch_bounds__(256) k_rec_partials(int64_t N, int64_t E, StressBatch sb)
{
    __shared__ double s_max[4 * 2];
    const int64_t v = blockIdx.y;
    const double *eta2 = sb.eta2 + v * E, *uterm = sb.uterm + v * E, *elem = sb.elem + v * 4 * E, *node = sb.node + v * 4 * N;
    double acc[2] = {0.0, 0.0}, mx[2] = {0.0, 0.0};
    share_sum(E, acc, [=](int64_t e, double (&a)[2]) {
        a[0] += eta2[e];
        a[1] += uterm[e];
    });
    share_sum(E, mx, [=](int64_t e, double (&a)[2]) { a[0] = fmax(a[0], elem[4 * e + 3]); });
    share_sum(N, mx, [=](int64_t i, double (&a)[2]) { a[1] = fmax(a[1], node[4 * i + 3]); });
    store_partials(acc, sb.partials);
    block_max256<2>(mx, s_max);
    if (threadIdx.x == 0) {
        double *out = sb.partials + 2 * ((int64_t)kSensBlocks * (sb.count + v) + blockIdx.x);
        out[0] = mx[0];
        out[1] = mx[1];
    }
}

// ---- ... stage two
__global__ void __launch_bounds__(256) k_rec_scalars(StressBatch sb)
{
    __shared__ double s_max[4 * 2];
    const double *in = sb.partials + 2 * ((int64_t)kSensBlocks * (sb.count + blockIdx.y) + threadIdx.x);
    double mx[2] = {in[0], in[1]};
    block_max256<2>(mx, s_max);
    sum_partials<2>(sb.partials, [&](int64_t v, const double (&acc)[2]) {
        double *out = sb.scalars + 8 * v;
        const double total = acc[1] + acc[0];
        out[0] = acc[0];
        out[1] = acc[1];
        out[2] = total > 0.0 ? sqrt(acc[0] / total) : 0.0;
        out[3] = mx[0];
        out[4] = mx[1];
        out[5] = out[6] = out[7] = 0.0;
    });
}

void stress_recovery(const SensMesh &m, const StressBatch &sb, hipStream_t s)
{
    const unsigned n = (unsigned)sb.count;
    const int64_t N = m.N, E = m.E;
    const dim3 per_element((unsigned)((E + 255) / 256), n);
    k_rec_elements<<<per_element, 256, 0, s>>>(m.conn, N, E, sb);
    if (m.tab)
        k_rec_nodes_tile<<<dim3((unsigned)m.T, n), 256, 32 * (size_t)m.cap, s>>>(m, sb);
    else
        k_rec_nodes<<<dim3((unsigned)((N + 255) / 256), n), 256, 0, s>>>(m, sb);
    k_rec_error<<<per_element, 256, 0, s>>>(m.conn, N, E, sb);
    k_rec_partials<<<dim3(kSensBlocks, n), 256, 0, s>>>(N, E, sb);
    k_rec_scalars<<<dim3(1, n), 256, 0, s>>>(sb);
}

} // namespace magk
