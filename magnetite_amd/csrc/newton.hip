// Nonlinear statics (mag_run_newton, mag_assemble_tangent): the device side of Newton's method on the total-Lagrangian internal
// force -- the consistent tangent in K's block-CSR pattern, the right-hand side with the support predictor, the norms of the stop
// rule, the update, the records.  The formulas are stated in newton.h.  Compiled -ffp-contract=off: the rounding is the source's
// (every multiply-add is the fma() it is written as); no floating-point atomics and every sum in a fixed order: a repeat gives the
// same bits, and so does every grid and every tile size.
#include "newton.h"
#include "member_pass.h"

namespace magk {

// ---- the tangent in the pattern: one thread per row node (Hilbert position g, caller id perm[g]), as k_tr_mass_pattern; the
// row itself is newton.h's tl_tangent_row, which transient_tl.hip finishes as the effective matrix
template <int LAW>
__global__ void __launch_bounds__(256) k_tl_tangent(TlMesh m, Pattern pat, const double2 *u, double *kval, int32_t *inverted)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= m.N) return;
    tl_tangent_row<LAW, false>(m, pat, u, g, kval, inverted, nullptr, 0.0, 0.0);
}

void tl_tangent(const TlMesh &m, const Pattern &pat, const double *u, double *kval, int32_t *inverted, hipStream_t s)
{
    (m.law == kLawNeoHooke ? k_tl_tangent<kLawNeoHooke> : k_tl_tangent<kLawSvk>)<<<dim3((unsigned)((m.N + 255) / 256)), 256, 0, s>>>(
        m, pat, (const double2 *)u, kval, inverted);
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

// ---- the per-element row: strains, stresses, det F and the strain energy, from the element's first corner (cs: the factor of
// tl_strain's s -- E / (1 - nu^2), under kLawNeoHooke mu)
template <int LAW>
__global__ void __launch_bounds__(256) k_nt_elements(TlMesh m, const double2 *u, double cs, double *elem, int32_t *inverted)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m.E) return;
    const int64_t a = m.conn[3 * e], b = m.conn[3 * e + 1], c = m.conn[3 * e + 2];
    const double2 ca = m.xy[a], cb = m.xy[b], cc = m.xy[c], ua = u[a], pb = u[b], pc = u[c];
    TlNeo neo;
    const TlStrain s = tl_strain<LAW>(make_double2(cb.x - ca.x, cb.y - ca.y), make_double2(pb.x - ua.x, pb.y - ua.y),
                                      make_double2(cc.x - ca.x, cc.y - ca.y), make_double2(pc.x - ua.x, pc.y - ua.y), m.nu, m.h, inverted, &neo);
    double *o = elem + 8 * e;
    o[0] = s.Exx;
    o[1] = s.Eyy;
    o[2] = s.Gxy;
    o[3] = cs * s.sx;
    o[4] = cs * s.sy;
    o[5] = cs * s.tq;
    o[6] = fma(1.0 + s.H11, 1.0 + s.H22, -(s.H12 * s.H21));
    if constexpr (LAW == kLawSvk)
        o[7] = tl_energy(s, m.c0);
    else
        o[7] = neo_energy(s, neo, m.c0, m.nu);
}

void newton_elements(const TlMesh &m, const double *u, double cs, double *elem, int32_t *inverted, hipStream_t s)
{
    (m.law == kLawNeoHooke ? k_nt_elements<kLawNeoHooke> : k_nt_elements<kLawSvk>)<<<dim3((unsigned)((m.E + 255) / 256)), 256, 0, s>>>(
        m, (const double2 *)u, cs, elem, inverted);
}

} // namespace magk
