// Modal analysis (mag_run_modal): the device side of the subspace iteration for K_FF phi = lambda M_FF phi -- the mass operator,
// the Gram matrices of the Rayleigh-Ritz step, the rotation of the subspace, the start vectors, the orientation check and the
// modes' residual norms and signs -- on the skeleton of member_pass.h: a pass over nodes, the two-stage reduction; per vector,
// the vector from blockIdx.y.  Vectors lie [count][2N] in the caller's numbering.  Compiled -ffp-contract=off: the rounding is
// the source's; no floating-point atomics: a repeat gives the same bits.
//
// With density rho, m_e = rho t |A_e| (|A_e|: the mass does not care about an element's orientation).  A triangle with corners
// (i, b, c) adds to row i, per direction,
//   consistent:  m_e / 12 (2 x_i + x_b + x_c)      (M_e = m_e / 12 [[2,1,1],[1,2,1],[1,1,2]]),
//   lumped:      m_e / 3 x_i,
// the sums in the order of the node's incidence list.
#include "modal.h"
#include "member_pass.h"

namespace magk {

namespace {

// The node pass of y = M x.  Fields: coordinates, x.
struct Mass {
    double c; // rho t
    int32_t lumped, masked;
    int64_t N;
    const uint8_t *known;
    double2 *y;
    struct Node {
        double x, y;
    };
    __device__ Mass(const Member &m, const MassBatch &mb, const SensMesh &mesh)
        : c(mb.density * m.thick), lumped(mb.lumped), masked(mb.masked), N(mesh.N), known(mesh.u_known), y((double2 *)mb.y)
    {
    }
    __device__ Node node(int64_t) const { return {0.0, 0.0}; }
    __device__ void corner(Node &n, const double2 (&f)[2][3], int32_t) const
    {
        const double me = c * (0.5 * fabs(edges_of(f[0]).A2));
        if (lumped) { // (the same for every thread of the launch)
            const double w = me / 3.0;
            n.x += w * f[1][0].x;
            n.y += w * f[1][0].y;
        } else {
            const double w = me / 12.0;
            n.x += w * ((2.0 * f[1][0].x + f[1][1].x) + f[1][2].x);
            n.y += w * ((2.0 * f[1][0].y + f[1][1].y) + f[1][2].y);
        }
    }
    __device__ void store(const Node &n, int64_t at) const
    {
        const int64_t id = at - (int64_t)blockIdx.y * N;
        const bool kx = masked != 0 && known[2 * id] != 0, ky = masked != 0 && known[2 * id + 1] != 0;
        y[at] = make_double2(kx ? 0.0 : n.x, ky ? 0.0 : n.y);
    }
};

// the finaliser of splitmix64
__device__ inline uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// in [-1, 1): stream c of the node whose coordinates hashed to `node` (53 bits of the hash: the conversion is exact)
__device__ inline double hash_unit(uint64_t node, uint32_t c)
{
    const uint64_t k = mix64(node + (uint64_t)(c + 1) * 0x9e3779b97f4a7c15ull);
    return (double)(k >> 11) / 4503599627370496.0 - 1.0;
}

} // namespace

// ---- y = M x, on the tile's image in LDS (32 * cap bytes, under 64 KiB at cap = kMaxLdsNodes) ...
__global__ void __launch_bounds__(256) k_modal_mass_tile(SensMesh mesh, MassBatch mb)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_img[];
    const Member m = member_of(mb, blockIdx.y, mesh.N);
    const double2 *const src[2] = {m.xy, m.u};
    tile_walk(mesh, src, s_img, Mass(m, mb, mesh));
}

// ---- ... or gathered from memory
__global__ void __launch_bounds__(256) k_modal_mass(SensMesh mesh, MassBatch mb)
{
    const Member m = member_of(mb, blockIdx.y, mesh.N);
    const double2 *const src[2] = {m.xy, m.u};
    gather_walk(mesh, src, Mass(m, mb, mesh));
}

void mass_apply(const SensMesh &m, const MassBatch &mb, hipStream_t s)
{
    const unsigned n = (unsigned)mb.count;
    if (m.tab)
        k_modal_mass_tile<<<dim3((unsigned)m.T, n), 256, 32 * (size_t)m.cap, s>>>(m, mb);
    else
        k_modal_mass<<<dim3((unsigned)((m.N + 255) / 256), n), 256, 0, s>>>(m, mb);
}

// ---- x = 0 on prescribed DOFs (mag_apply_mass masked: the columns of P)
__global__ void __launch_bounds__(256) k_modal_mask(const uint8_t *known, int64_t n2, double *x)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d < n2) x[blockIdx.y * n2 + d] = known[d] ? 0.0 : x[blockIdx.y * n2 + d];
}

void mask_vectors(const uint8_t *u_known, int64_t N, int32_t count, double *X, hipStream_t s)
{
    k_modal_mask<<<dim3((unsigned)((2 * N + 255) / 256), (unsigned)count), 256, 0, s>>>(u_known, 2 * N, X);
}

// ---- the Gram matrices, stage one: workgroup row i * JC + jc sums z_i . y_j and z_i . w_j for the kModalGramCols columns j from
// kModalGramCols * jc (a column past q - 1 repeats column q - 1 and is dropped by stage two)
__global__ void __launch_bounds__(256) k_modal_gram_partials(const double2 *Z, const double2 *Y, const double2 *W, int64_t N, int32_t q,
                                                             double *partials)
{
    constexpr int C = kModalGramCols;
    const int32_t JC = (q + C - 1) / C, i = (int32_t)blockIdx.y / JC, j0 = C * ((int32_t)blockIdx.y % JC);
    const double2 *zi = Z + (int64_t)i * N;
    const double2 *yj[C], *wj[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t j = j0 + c < q ? j0 + c : q - 1;
        yj[c] = Y + j * N;
        wj[c] = W + j * N;
    }
    double acc[2 * C];
#pragma unroll
    for (int c = 0; c < 2 * C; ++c) acc[c] = 0.0;
    share_sum(N, acc, [=](int64_t n, double (&a)[2 * C]) {
        const double2 z = zi[n];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double2 y = yj[c][n], w = wj[c][n];
            a[2 * c] += z.x * y.x;
            a[2 * c] += z.y * y.y;
            a[2 * c + 1] += z.x * w.x;
            a[2 * c + 1] += z.y * w.y;
        }
    });
    store_partials(acc, partials);
}

// ---- ... stage two: out = A (q x q), then B
__global__ void __launch_bounds__(256) k_modal_gram_sum(const double *partials, int32_t q, double *out)
{
    constexpr int C = kModalGramCols;
    sum_partials<2 * C>(partials, [&](int64_t v, const double (&acc)[2 * C]) {
        const int32_t JC = (q + C - 1) / C, i = (int32_t)v / JC, j0 = C * ((int32_t)v % JC);
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (j0 + c < q) {
                out[i * q + j0 + c] = acc[2 * c];
                out[q * q + i * q + j0 + c] = acc[2 * c + 1];
            }
    });
}

void gram(const double *Z, const double *Y, const double *W, int64_t N, int32_t q, double *partials, double *out, hipStream_t s)
{
    const unsigned rows = (unsigned)gram_rows(q);
    k_modal_gram_partials<<<dim3(kSensBlocks, rows), 256, 0, s>>>((const double2 *)Z, (const double2 *)Y, (const double2 *)W, N, q, partials);
    k_modal_gram_sum<<<dim3(1, rows), 256, 0, s>>>(partials, q, out);
}

// ---- the rotation: one thread per DOF d reads its q inputs once per product (QC >= q of them in registers, zeros past q) and
// writes the q outputs; Q and lambda come from LDS.  With R, R_k = (Yold Q)_k first, then R_k -= lambda_k Ynew_k once Ynew_k is
// there (the thread's own entry of R).
template <int QC>
__global__ void __launch_bounds__(256) k_modal_rotate(const double *Z, const double *W, const double *Yold, const double *qs, int64_t n2,
                                                      int32_t q, int32_t modes, double *X, double *Ynew, double *R)
{
    __shared__ double s_q[kModalMaxQ * kModalMaxQ + kModalMaxQ];
    for (int i = threadIdx.x; i < kModalMaxQ * kModalMaxQ + kModalMaxQ; i += 256) s_q[i] = qs[i];
    __syncthreads();
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n2) return;
    const double *lambda = s_q + kModalMaxQ * kModalMaxQ;
    double a[QC];
#pragma unroll
    for (int j = 0; j < QC; ++j) a[j] = j < q ? Z[j * n2 + d] : 0.0;
    for (int32_t k = 0; k < q; ++k) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < QC; ++j) sum += a[j] * s_q[j * kModalMaxQ + k];
        X[k * n2 + d] = sum;
    }
    if (R) { // (the same for every thread of the launch)
#pragma unroll
        for (int j = 0; j < QC; ++j) a[j] = j < q ? Yold[j * n2 + d] : 0.0;
        for (int32_t k = 0; k < modes; ++k) {
            double sum = 0.0;
#pragma unroll
            for (int j = 0; j < QC; ++j) sum += a[j] * s_q[j * kModalMaxQ + k];
            R[k * n2 + d] = sum;
        }
    }
#pragma unroll
    for (int j = 0; j < QC; ++j) a[j] = j < q ? W[j * n2 + d] : 0.0;
    for (int32_t k = 0; k < q; ++k) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < QC; ++j) sum += a[j] * s_q[j * kModalMaxQ + k];
        Ynew[k * n2 + d] = sum;
        if (R && k < modes) R[k * n2 + d] = R[k * n2 + d] - lambda[k] * sum;
    }
}

void rotate(const double *Z, const double *W, const double *Yold, const double *qs, int64_t N, int32_t q, int32_t modes, double *X,
            double *Ynew, double *R, hipStream_t s)
{
    const int64_t n2 = 2 * N;
    const dim3 g((unsigned)((n2 + 255) / 256));
    if (q <= 8)
        k_modal_rotate<8><<<g, 256, 0, s>>>(Z, W, Yold, qs, n2, q, modes, X, Ynew, R);
    else if (q <= 16)
        k_modal_rotate<16><<<g, 256, 0, s>>>(Z, W, Yold, qs, n2, q, modes, X, Ynew, R);
    else if (q <= 24)
        k_modal_rotate<24><<<g, 256, 0, s>>>(Z, W, Yold, qs, n2, q, modes, X, Ynew, R);
    else
        k_modal_rotate<32><<<g, 256, 0, s>>>(Z, W, Yold, qs, n2, q, modes, X, Ynew, R);
}

// ---- |R_k|^2 and |Y_k|^2, the two stages
__global__ void __launch_bounds__(256) k_modal_norm_partials(const double *R, const double *Y, int64_t n2, double *partials)
{
    const double *r = R + (int64_t)blockIdx.y * n2, *y = Y + (int64_t)blockIdx.y * n2;
    double acc[2] = {0.0, 0.0};
    share_sum(n2, acc, [=](int64_t i, double (&a)[2]) {
        a[0] += r[i] * r[i];
        a[1] += y[i] * y[i];
    });
    store_partials(acc, partials);
}

__global__ void __launch_bounds__(256) k_modal_norm_sum(const double *partials, double *out)
{
    sum_partials<2>(partials, [&](int64_t v, const double (&acc)[2]) {
        out[2 * v] = acc[0];
        out[2 * v + 1] = acc[1];
    });
}

void residual_norms(const double *R, const double *Y, int64_t N, int32_t modes, double *partials, double *out, hipStream_t s)
{
    k_modal_norm_partials<<<dim3(kSensBlocks, (unsigned)modes), 256, 0, s>>>(R, Y, 2 * N, partials);
    k_modal_norm_sum<<<dim3(1, (unsigned)modes), 256, 0, s>>>(partials, out);
}

// ---- the start vectors: a function of the uploaded coordinates and the vector's index only -- a fixed integer hash of the
// bits of the node's coordinates (+ 0.0: a -0 counts as 0) and of 2 j + direction, mapped to [-1, 1).  No polynomial of the
// coordinates: nothing degenerates on a mesh one element thick, and the q vectors are as good as orthogonal
__global__ void __launch_bounds__(256) k_modal_start(const double2 *xy, const uint8_t *known, int64_t N, double2 *X)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t j = blockIdx.y;
    if (i >= N) return;
    const double2 c = xy[i];
    const uint64_t node = mix64(mix64((uint64_t)__double_as_longlong(c.x + 0.0) + 0x9e3779b97f4a7c15ull) ^ (uint64_t)__double_as_longlong(c.y + 0.0));
    X[(int64_t)j * N + i] = make_double2(known[2 * i] ? 0.0 : hash_unit(node, 2 * j), known[2 * i + 1] ? 0.0 : hash_unit(node, 2 * j + 1));
}

void start_vectors(const double *xy, const uint8_t *u_known, int64_t N, int32_t q, double *X, hipStream_t s)
{
    k_modal_start<<<dim3((unsigned)((N + 255) / 256), (unsigned)q), 256, 0, s>>>((const double2 *)xy, u_known, N, (double2 *)X);
}

// ---- the reference's K_e carries the SIGNED area: an element of area <= 0 makes K indefinite.  The first offender by an atomic
// (integer) minimum -- offenders only
__global__ void __launch_bounds__(256) k_modal_orientation(const double2 *xy, const int32_t *conn, int64_t N, int64_t E, unsigned long long *bad)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
    if ((uint32_t)n0 >= (uint64_t)N || (uint32_t)n1 >= (uint64_t)N || (uint32_t)n2 >= (uint64_t)N) return; // (the ordering phase reports it)
    const double2 c[3] = {xy[n0], xy[n1], xy[n2]};
    if (!(edges_of(c).A2 > 0.0)) atomicMin(bad, (unsigned long long)e);
}

void orientation(const double *xy, const int32_t *conn, int64_t N, int64_t E, unsigned long long *bad, hipStream_t s)
{
    (void)hipMemsetAsync(bad, 0xff, 8, s);
    k_modal_orientation<<<dim3((unsigned)((E + 255) / 256)), 256, 0, s>>>((const double2 *)xy, conn, N, E, bad);
}

// ---- the sign convention of a mode: its entry of largest magnitude is positive, on a tie the first in caller order.  One
// workgroup per vector: every thread's candidate (strictly larger wins: the first of its entries), then a tree over the 256
// candidates in LDS (larger magnitude, then smaller index), every thread taking part in every step
__global__ void __launch_bounds__(256) k_modal_sign(double *X, int64_t n2)
{
    __shared__ double s_a[256];
    __shared__ int64_t s_i[256];
    double *x = X + (int64_t)blockIdx.x * n2;
    double best = -1.0;
    int64_t at = n2;
    for (int64_t i = threadIdx.x; i < n2; i += 256) {
        const double a = fabs(x[i]);
        const bool take = a > best;
        best = take ? a : best;
        at = take ? i : at;
    }
    s_a[threadIdx.x] = best;
    s_i[threadIdx.x] = at;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        const int o = (int)threadIdx.x + off < 256 ? (int)threadIdx.x + off : (int)threadIdx.x;
        const double a0 = s_a[threadIdx.x], a1 = s_a[o];
        const int64_t i0 = s_i[threadIdx.x], i1 = s_i[o];
        const bool take = a1 > a0 || (a1 == a0 && i1 < i0);
        __syncthreads();
        s_a[threadIdx.x] = take ? a1 : a0;
        s_i[threadIdx.x] = take ? i1 : i0;
        __syncthreads();
    }
    const int64_t top = s_i[0];
    const bool flip = top < n2 && x[top] < 0.0;
    __syncthreads(); // (every thread has read the deciding entry before any thread changes it)
    if (flip) // (the same for every thread of the workgroup)
        for (int64_t i = threadIdx.x; i < n2; i += 256) x[i] = 0.0 - x[i]; // (a zero stays +0)
}

void fix_signs(double *X, int64_t N, int32_t modes, hipStream_t s)
{
    k_modal_sign<<<dim3((unsigned)modes), 256, 0, s>>>(X, 2 * N);
}

} // namespace magk
