// Nonlinear statics (mag_run_newton, mag_assemble_tangent): the device side of Newton's method on the total-Lagrangian internal
// force -- the consistent tangent in K's block-CSR pattern, the right-hand side with the support predictor, the norms of the stop
// rule, the update, the records.  The formulas are stated in newton.h.  Compiled -ffp-contract=off: the rounding is the source's
// (every multiply-add is the fma() it is written as); no floating-point atomics and every sum in a fixed order: a repeat gives the
// same bits, and so does every grid and every tile size.
#include "newton.h"
#include "member_pass.h"

namespace magk {

// ---- the tangent in the pattern: one thread per row node (Hilbert position g, caller id perm[g]), as k_tr_mass_pattern.  The
// row's values are zeroed, then every incident triangle adds its three blocks of this node's row, in list order.  The triangle is
// always taken from its first corner on, so that its three rows see the same H, F and S.
__global__ void __launch_bounds__(256) k_tl_tangent(TlMesh m, Pattern pat, const double2 *u, double *kval, int32_t *inverted)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= m.N) return;
    const int64_t i = m.perm[g];
    const int32_t p = pat.bptr[i], cnt = pat.bptr[i + 1] - p;
    double *row0 = kval + 4 * (int64_t)p, *row1 = row0 + 2 * cnt;
    for (int32_t k = 0; k < 2 * cnt; ++k) row0[k] = 0.0, row1[k] = 0.0;
    const double nu = m.nu, h = m.h;
    const int32_t q1 = m.inc_off[g + 1];
    for (int32_t q = m.inc_off[g]; q < q1; ++q) {
        const uint32_t w = m.inc[q];
        const int64_t e = w / 3u;
        const int a = (int)(w - 3u * (uint32_t)e);
        const int32_t n0 = m.conn[3 * e], n1 = m.conn[3 * e + 1], n2 = m.conn[3 * e + 2];
        const double2 x0 = m.xy[n0], x1 = m.xy[n1], x2 = m.xy[n2], u0 = u[n0], u1 = u[n1], u2 = u[n2];
        const double2 db = make_double2(x1.x - x0.x, x1.y - x0.y), dc = make_double2(x2.x - x0.x, x2.y - x0.y);
        const TlStrain s = tl_strain(db, make_double2(u1.x - u0.x, u1.y - u0.y), dc, make_double2(u2.x - u0.x, u2.y - u0.y), nu, h, inverted);
        const double r = ring_rcp<double>(s.twoA);
        const double2 g0 = make_double2((db.y - dc.y) * r, (dc.x - db.x) * r), g1 = make_double2(dc.y * r, -(dc.x * r)),
                      g2 = make_double2(-(db.y * r), db.x * r);
        const double F11 = 1.0 + s.H11, F12 = s.H12, F21 = s.H21, F22 = 1.0 + s.H22;
        const double wv = s.twoA * m.c0; // V c
        const double2 gk = a == 0 ? g0 : (a == 1 ? g1 : g2);
        // (D / c) B_k, column d: (p0 + nu p1, p1 + nu p0, h p2) of p = (F_d1 gk.x, F_d2 gk.y, F_d1 gk.y + F_d2 gk.x)
        const double pa0 = F11 * gk.x, pa1 = F12 * gk.y, pa2 = fma(F11, gk.y, F12 * gk.x);
        const double pb0 = F21 * gk.x, pb1 = F22 * gk.y, pb2 = fma(F21, gk.y, F22 * gk.x);
        const double da0 = fma(nu, pa1, pa0), da1 = fma(nu, pa0, pa1), da2 = h * pa2;
        const double db0 = fma(nu, pb1, pb0), db1 = fma(nu, pb0, pb1), db2 = h * pb2;
        // (S / c) g_k
        const double tx = fma(s.sx, gk.x, s.tq * gk.y), ty = fma(s.tq, gk.x, s.sy * gk.y);
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const double2 gl = l == 0 ? g0 : (l == 1 ? g1 : g2);
            const int32_t j = l == 0 ? n0 : (l == 1 ? n1 : n2);
            const double qa0 = F11 * gl.x, qa1 = F12 * gl.y, qa2 = fma(F11, gl.y, F12 * gl.x);
            const double qb0 = F21 * gl.x, qb1 = F22 * gl.y, qb2 = fma(F21, gl.y, F22 * gl.x);
            const double geo = fma(tx, gl.x, ty * gl.y);
            const double k00 = wv * (fma(da0, qa0, fma(da1, qa1, da2 * qa2)) + geo);
            const double k01 = wv * fma(da0, qb0, fma(da1, qb1, da2 * qb2));
            const double k10 = wv * fma(db0, qa0, fma(db1, qa1, db2 * qa2));
            const double k11 = wv * (fma(db0, qb0, fma(db1, qb1, db2 * qb2)) + geo);
            for (int32_t k = 0; k < cnt; ++k) // (the column is one of the row's: K couples the same pairs)
                if (pat.bcol[p + k] == j) {
                    row0[2 * k] = row0[2 * k] + k00;
                    row0[2 * k + 1] = row0[2 * k + 1] + k01;
                    row1[2 * k] = row1[2 * k] + k10;
                    row1[2 * k + 1] = row1[2 * k + 1] + k11;
                    break;
                }
        }
    }
}

void tl_tangent(const TlMesh &m, const Pattern &pat, const double *u, double *kval, int32_t *inverted, hipStream_t s)
{
    k_tl_tangent<<<dim3((unsigned)((m.N + 255) / 256)), 256, 0, s>>>(m, pat, (const double2 *)u, kval, inverted);
}

// ---- the right-hand side: one thread per DOF, the row in ascending column order
__global__ void __launch_bounds__(256) k_nt_rhs(Pattern pat, const double *kval, const uint8_t *known, const double *f, const double *load,
                                                int64_t at, const double *fint, const double *u, const double *u_in, int32_t first,
                                                double *rhs, double *dup)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= 2 * pat.N) return;
    const double lam = load[at];
    const bool fixed = known[r] != 0;
    double sk = 0.0;
    if (first) {
        const int64_t i = r >> 1;
        const int d = (int)(r & 1);
        const int32_t p = pat.bptr[i], cnt = pat.bptr[i + 1] - p;
        const double *row = kval + 4 * (int64_t)p + (int64_t)d * 2 * cnt;
        for (int32_t k = 0; k < cnt; ++k) {
            const int64_t j = pat.bcol[p + k];
            const double x0 = known[2 * j] ? lam * u_in[2 * j] - u[2 * j] : 0.0;
            const double x1 = known[2 * j + 1] ? lam * u_in[2 * j + 1] - u[2 * j + 1] : 0.0;
            sk += row[2 * k] * x0;
            sk += row[2 * k + 1] * x1;
        }
        dup[r] = fixed ? lam * u_in[r] - u[r] : 0.0;
    }
    rhs[r] = fixed ? 0.0 : (lam * f[r] - fint[r]) - sk;
}

void newton_rhs(const Pattern &pat, const double *kval, const uint8_t *known, const double *f, const double *load, int64_t at,
                const double *fint, const double *u, const double *u_in, int32_t first, double *rhs, double *dup, hipStream_t s)
{
    k_nt_rhs<<<dim3((unsigned)((2 * pat.N + 255) / 256)), 256, 0, s>>>(pat, kval, known, f, load, at, fint, u, u_in, first, rhs, dup);
}

// ---- the norms of the stop rule, the load's work and the slope of the line search, the two stages
__global__ void __launch_bounds__(256) k_nt_norm_partials(const uint8_t *known, const double *f, const double *load, int64_t at,
                                                          const double *fint, const double *u, const double *du, int64_t n2, double *partials)
{
    const double lam = load[at];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    share_sum(n2, acc, [&](int64_t i, double (&a)[5]) {
        const bool fixed = known[i] != 0;
        const double lf = fixed ? 0.0 : lam * f[i], fi = fint[i];
        const double r = fixed ? 0.0 : lf - fi;
        a[0] += r * r;
        a[1] += lf * lf;
        a[2] += fixed ? fi * fi : 0.0;
        a[3] += fixed ? 0.0 : f[i] * u[i];
        if (du) a[4] += (fi - lf) * du[i];
    });
    store_partials(acc, partials);
}

__global__ void __launch_bounds__(256) k_nt_norm_sum(const double *partials, NewtonScalars *out)
{
    sum_partials<5>(partials, [&](int64_t, const double (&acc)[5]) {
        out->r2 = acc[0];
        out->f2 = acc[1];
        out->p2 = acc[2];
        out->fu = acc[3];
        out->slope = acc[4];
    });
}

void newton_norms(const uint8_t *known, const double *f, const double *load, int64_t at, const double *fint, const double *u,
                  const double *du, int64_t n2, double *partials, NewtonScalars *out, hipStream_t s)
{
    k_nt_norm_partials<<<dim3(kSensBlocks, 1), 256, 0, s>>>(known, f, load, at, fint, u, du, n2, partials);
    k_nt_norm_sum<<<dim3(1, 1), 256, 0, s>>>(partials, out);
}

// ---- the update
__global__ void __launch_bounds__(256) k_nt_update(const double *u, const double *du, double s, int64_t n2, double *out)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d < n2) out[d] = u[d] + s * du[d];
}

void newton_update(const double *u, const double *du, double s, int64_t n2, double *out, hipStream_t s_)
{
    k_nt_update<<<dim3((unsigned)((n2 + 255) / 256)), 256, 0, s_>>>(u, du, s, n2, out);
}

// ---- the records of a converged increment: the probes by threads of their own behind the 2N of the snapshot
__global__ void __launch_bounds__(256) k_nt_record(const double *u, const int32_t *probes, int32_t num_probes, int64_t row, double *probe_u,
                                                   double *snap, int64_t n2)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n2) {
        if (snap) snap[t] = u[t];
    } else if (t - n2 < num_probes) {
        probe_u[row * num_probes + (t - n2)] = u[probes[t - n2]];
    }
}

void newton_record(const double *u, const int32_t *probes, int32_t num_probes, int64_t row, double *probe_u, double *snap, int64_t n2,
                   hipStream_t s)
{
    k_nt_record<<<dim3((unsigned)((n2 + num_probes + 255) / 256)), 256, 0, s>>>(u, probes, num_probes, row, probe_u, snap, n2);
}

// ---- the per-element row: strains, stresses, det F and the strain energy, from the element's first corner
__global__ void __launch_bounds__(256) k_nt_elements(TlMesh m, const double2 *u, double cs, double *elem, int32_t *inverted)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m.E) return;
    const int64_t a = m.conn[3 * e], b = m.conn[3 * e + 1], c = m.conn[3 * e + 2];
    const double2 ca = m.xy[a], cb = m.xy[b], cc = m.xy[c], ua = u[a], pb = u[b], pc = u[c];
    const TlStrain s = tl_strain(make_double2(cb.x - ca.x, cb.y - ca.y), make_double2(pb.x - ua.x, pb.y - ua.y),
                                 make_double2(cc.x - ca.x, cc.y - ca.y), make_double2(pc.x - ua.x, pc.y - ua.y), m.nu, m.h, inverted);
    double *o = elem + 8 * e;
    o[0] = s.Exx;
    o[1] = s.Eyy;
    o[2] = s.Gxy;
    o[3] = cs * s.sx;
    o[4] = cs * s.sy;
    o[5] = cs * s.tq;
    o[6] = fma(1.0 + s.H11, 1.0 + s.H22, -(s.H12 * s.H21));
    o[7] = tl_energy(s, m.c0);
}

void newton_elements(const TlMesh &m, const double *u, double cs, double *elem, int32_t *inverted, hipStream_t s)
{
    k_nt_elements<<<dim3((unsigned)((m.E + 255) / 256)), 256, 0, s>>>(m, (const double2 *)u, cs, elem, inverted);
}

} // namespace magk
