// Linearised buckling (mag_run_buckling, mag_apply_geometric, mag_assemble_geometric): the geometric stiffness K_G(sigma(u0)) of a
// solved member -- as an operator on many vectors on the skeleton of member_pass.h (a pass over nodes; per vector, the vector from
// blockIdx.y) and as values in K's block-CSR pattern.  The formulas are stated in buckling.h.  The rest of the subspace iteration
// (Gram matrices, rotation, norms, signs, start vectors, orientation) is modal.hip's.  Compiled -ffp-contract=off: the rounding is
// the source's; no floating-point atomics: a repeat gives the same bits, and so does every grid.
#include "buckling.h"
#include "member_pass.h"

namespace magk {

namespace {

// Coordinates and u0 enter as differences to the triangle's first corner (c_k - c_0, u_k - u_0: b, g and the tensor do not see a
// translation).  The cyclic sums of a small triangle far from the origin cancel -- A2 = sum x_i b_i to h^2 out of terms of size h,
// the strains to |du| out of terms of size |u| --, which on a jittered mesh of 3k nodes costs K_G 1e-13 of its largest entry; the
// differences are exact to rounding and leave 4e-16 (tests/test_buckling_gpu.py holds the operator to 1e-14).
__device__ inline void to_first_corner(const double2 (&v)[3], double2 (&d)[3])
{
    d[0] = make_double2(0.0, 0.0);
    d[1] = make_double2(v[1].x - v[0].x, v[1].y - v[0].y);
    d[2] = make_double2(v[2].x - v[0].x, v[2].y - v[0].y);
}

// sigma_e of the prestress (recover.hip's tensor_of, the same expressions) and w = t / (2 A2)
struct Prestress {
    double sx, sy, txy, w;
};

__device__ inline Prestress prestress_of(const Edges &e, const double2 (&u)[3], double nu, double cs, double half_t)
{
    const Sums s = cyclic_sums(e, u);
    const double ci = cs / e.A2;
    return {ci * (s.p + nu * s.q), ci * (nu * s.p + s.q), ci * (0.5 * (1.0 - nu) * s.r), half_t / e.A2};
}

// h_kl for l = 0, 1, 2: t A_e (g_k^T sigma g_l), with (bk, gk) = (e.b[k], e.g[k])
__device__ inline void coefficients(const Edges &e, const Prestress &p, double bk, double gk, double (&h)[3])
{
    const double tx = p.sx * bk + p.txy * gk, ty = p.txy * bk + p.sy * gk;
#pragma unroll
    for (int l = 0; l < 3; ++l) h[l] = p.w * (tx * e.b[l] + ty * e.g[l]);
}

// The node pass of y = sign K_G x.  Fields: coordinates, u0, x.
struct Geometric {
    double nu, cs, half_t, sign;
    int32_t masked;
    int64_t N;
    const uint8_t *known;
    double2 *y;
    struct Node {
        double x, y;
    };
    __device__ Geometric(const Member &m, const GeomBatch &gb, const SensMesh &mesh)
        : nu(m.nu), cs(m.youngs / (1.0 - m.nu * m.nu)), half_t(0.5 * m.thick), sign(gb.sign), masked(gb.masked), N(mesh.N),
          known(mesh.u_known), y((double2 *)gb.y)
    {
    }
    __device__ Node node(int64_t) const { return {0.0, 0.0}; }
    __device__ void corner(Node &n, const double2 (&f)[3][3], int32_t) const
    {
        double2 c[3], u[3];
        to_first_corner(f[0], c);
        to_first_corner(f[1], u);
        const Edges e = edges_of(c);
        const Prestress p = prestress_of(e, u, nu, cs, half_t);
        double h[3];
        coefficients(e, p, e.b[0], e.g[0], h);
        n.x += (h[0] * f[2][0].x + h[1] * f[2][1].x) + h[2] * f[2][2].x;
        n.y += (h[0] * f[2][0].y + h[1] * f[2][1].y) + h[2] * f[2][2].y;
    }
    __device__ void store(const Node &n, int64_t at) const
    {
        const int64_t id = at - (int64_t)blockIdx.y * N;
        const bool kx = masked != 0 && known[2 * id] != 0, ky = masked != 0 && known[2 * id + 1] != 0;
        y[at] = make_double2(kx ? 0.0 : sign * n.x, ky ? 0.0 : sign * n.y);
    }
};

} // namespace

// ---- y = sign K_G x, on the tile's image in LDS: 48 * cap bytes, up to 96768 at cap = kMaxLdsNodes (the launch wrapper raises the
// 64 KiB default limit, as adjoint.hip's does) ...
__global__ void __launch_bounds__(256) k_buckling_geometric_tile(SensMesh mesh, GeomBatch gb)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    const Member m = member_of(gb, blockIdx.y, mesh.N);
    const double2 *const src[3] = {m.xy, (const double2 *)gb.u0, m.u};
    tile_walk(mesh, src, s_img, Geometric(m, gb, mesh));
}

// ---- ... or gathered from memory
__global__ void __launch_bounds__(256) k_buckling_geometric(SensMesh mesh, GeomBatch gb)
{
    const Member m = member_of(gb, blockIdx.y, mesh.N);
    const double2 *const src[3] = {m.xy, (const double2 *)gb.u0, m.u};
    gather_walk(mesh, src, Geometric(m, gb, mesh));
}

hipError_t geometric_apply(const SensMesh &m, const GeomBatch &gb, hipStream_t s)
{
    const unsigned n = (unsigned)gb.count;
    if (m.tab) {
        const size_t lds = 48 * (size_t)m.cap; // cap <= kMaxLdsNodes: at most 96768 of the CU's 160 KiB
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute((const void *)k_buckling_geometric_tile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        k_buckling_geometric_tile<<<dim3((unsigned)m.T, n), 256, lds, s>>>(m, gb);
    } else {
        k_buckling_geometric<<<dim3((unsigned)((m.N + 255) / 256), n), 256, 0, s>>>(m, gb);
    }
    return hipSuccess;
}

// ---- K_G in the pattern: one thread per row node (Hilbert position g, caller id perm[g]), k_tl_tangent's row walk without the
// material term -- the row's values are zeroed, then every incident triangle, taken from its first corner on (its three rows see
// the same sigma), adds h_al to the diagonals of its three blocks of this node's row (one scan of the row's columns), in list order
__global__ void __launch_bounds__(256) k_buckling_values(SensMesh m, Pattern pat, const double2 *xy, const double *mat, const double2 *u0,
                                                         double *val)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= m.N) return;
    const int64_t i = m.perm[g];
    const int32_t p = pat.bptr[i], cnt = pat.bptr[i + 1] - p;
    double *row0 = val + 4 * (int64_t)p, *row1 = row0 + 2 * cnt;
    for (int32_t k = 0; k < 2 * cnt; ++k) row0[k] = 0.0, row1[k] = 0.0;
    const double nu = mat[1], cs = mat[0] / (1.0 - nu * nu), half_t = 0.5 * mat[2];
    const int32_t q1 = m.inc_off[g + 1];
    for (int32_t q = m.inc_off[g]; q < q1; ++q) {
        const uint32_t w = m.inc[q];
        const int64_t e = w / 3u;
        const int a = (int)(w - 3u * (uint32_t)e);
        const int32_t n0 = m.conn[3 * e], n1 = m.conn[3 * e + 1], n2 = m.conn[3 * e + 2];
        const double2 cn[3] = {xy[n0], xy[n1], xy[n2]}, un[3] = {u0[n0], u0[n1], u0[n2]};
        double2 c[3], u[3];
        to_first_corner(cn, c);
        to_first_corner(un, u);
        const Edges ed = edges_of(c);
        const Prestress ps = prestress_of(ed, u, nu, cs, half_t);
        double h[3];
        // (selects, not an indexed array: nothing goes to scratch)
        coefficients(ed, ps, a == 0 ? ed.b[0] : (a == 1 ? ed.b[1] : ed.b[2]), a == 0 ? ed.g[0] : (a == 1 ? ed.g[1] : ed.g[2]), h);
        for (int32_t k = 0; k < cnt; ++k) { // (the triangle's three columns are among the row's: K couples the same pairs)
            const int32_t j = pat.bcol[p + k];
            if (j != n0 && j != n1 && j != n2) continue;
            const double hl = j == n0 ? h[0] : (j == n1 ? h[1] : h[2]);
            row0[2 * k] = row0[2 * k] + hl;
            row1[2 * k + 1] = row1[2 * k + 1] + hl;
        }
    }
}

void geometric_values(const SensMesh &m, const Pattern &pat, const double *xy, const double *mat, const double *u0, double *val,
                      hipStream_t s)
{
    k_buckling_values<<<dim3((unsigned)((m.N + 255) / 256)), 256, 0, s>>>(m, pat, (const double2 *)xy, mat, (const double2 *)u0, val);
}

} // namespace magk
