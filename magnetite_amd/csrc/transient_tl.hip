// Nonlinear transient dynamics (mag_run_transient_tl, mag_assemble_effective_tangent): the device side of Newmark's method on
// the total-Lagrangian internal force with Newton's method in every step -- the effective tangent in K's block-CSR pattern, the
// trial state, the residual with the norms of the stop rule, the reactions and the energy row.  The method is stated in
// transient_tl.h.  Compiled -ffp-contract=off: the rounding is the source's (every multiply-add is the fma() it is written as); no
// floating-point atomics and every sum in a fixed order: a repeat gives the same bits, and a resumed run the bits of the run it
// continues.
#include "transient_tl.h"
#include "member_pass.h"

namespace magk {

// ---- A_T = c_K K_T(u) + c_M M: k_tl_tangent with the row finished by its lane
template <int LAW>
__global__ void __launch_bounds__(256) k_tt_effective_tangent(TlMesh m, Pattern pat, const double2 *u, const double *mval, double c_K, double c_M,
                                                              double *aval, int32_t *inverted)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= m.N) return;
    tl_tangent_row<LAW, true>(m, pat, u, g, aval, inverted, mval, c_K, c_M);
}

void tl_effective_tangent(const TlMesh &m, const Pattern &pat, const double *u, const double *mval, double c_K, double c_M, double *aval,
                          int32_t *inverted, hipStream_t s)
{
    (m.law == kLawNeoHooke ? k_tt_effective_tangent<kLawNeoHooke> : k_tt_effective_tangent<kLawSvk>)<<<dim3((unsigned)((m.N + 255) / 256)), 256, 0, s>>>(
        m, pat, (const double2 *)u, mval, c_K, c_M, aval, inverted);
}

// ---- the trial state: one thread per DOF
__global__ void __launch_bounds__(256) k_tt_trial(TlTrial t, double s_len, double c_u, double c_v, int32_t first)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= t.n2) return;
    const double ut = t.ut[d], vt = t.vt[d];
    double an;
    if (first)
        an = t.known[d] ? 0.0 : (t.u[d] - ut) / c_u;
    else
        an = fma(s_len, t.da[d], t.a_it[d]);
    t.an[d] = an;
    t.un[d] = fma(c_u, an, ut);
    t.vn[d] = fma(c_v, an, vt);
}

void tl_trial_state(const TlTrial &t, double s_len, double c_u, double c_v, int32_t first, hipStream_t s)
{
    k_tt_trial<<<dim3((unsigned)((t.n2 + 255) / 256)), 256, 0, s>>>(t, s_len, c_u, c_v, first);
}

// (M (a + alpha v))[r], the row in ascending column order
__device__ inline double inertia_row(const Pattern &pat, const double *mval, int64_t r, const double *a, const double *v, double alpha)
{
    const int64_t i = r >> 1;
    const int d = (int)(r & 1);
    double sm = 0.0;
    for (int32_t p = pat.bptr[i]; p < pat.bptr[i + 1]; ++p) {
        const int64_t c = 2 * (int64_t)pat.bcol[p] + d;
        sm = fma(mval[p], fma(alpha, v[c], a[c]), sm);
    }
    return sm;
}

// ---- the residual and stage one of its norms: each lane its fixed share of the 2N rows
__global__ void __launch_bounds__(256) k_tt_residual(Pattern pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude,
                                                     int64_t amp_at, const double *fint, const double *a, const double *v, double alpha, double *r,
                                                     double *partials)
{
    const double amp = amplitude[amp_at];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    share_sum(2 * pat.N, acc, [&](int64_t i, double (&s)[4]) {
        if (known[i]) {
            r[i] = 0.0;
            return;
        }
        const double lf = amp * f[i], fi = fint[i], mi = inertia_row(pat, mval, i, a, v, alpha);
        const double ri = (lf - fi) - mi;
        r[i] = ri;
        s[0] = fma(ri, ri, s[0]);
        s[1] = fma(lf, lf, s[1]);
        s[2] = fma(fi, fi, s[2]);
        s[3] = fma(mi, mi, s[3]);
    });
    store_partials(acc, partials);
}

__global__ void __launch_bounds__(256) k_tt_residual_sum(const double *partials, TlStepScalars *out)
{
    sum_partials<4>(partials, [&](int64_t, const double (&acc)[4]) {
        out->r2 = acc[0];
        out->f2 = acc[1];
        out->i2 = acc[2];
        out->m2 = acc[3];
    });
}

void tl_residual(const Pattern &pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude, int64_t amp_at,
                 const double *fint, const double *a, const double *v, double alpha, double *r, double *partials, TlStepScalars *out,
                 hipStream_t s)
{
    k_tt_residual<<<dim3(kSensBlocks, 1), 256, 0, s>>>(pat, mval, known, f, amplitude, amp_at, fint, a, v, alpha, r, partials);
    k_tt_residual_sum<<<dim3(1, 1), 256, 0, s>>>(partials, out);
}

// ---- the reactions: one thread per DOF
__global__ void __launch_bounds__(256) k_tt_reactions(Pattern pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude,
                                                      int64_t amp_at, const double *fint, const double *a, const double *v, double alpha, double *out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= 2 * pat.N) return;
    out[r] = known[r] ? fint[r] + inertia_row(pat, mval, r, a, v, alpha) : amplitude[amp_at] * f[r];
}

void tl_dynamic_reactions(const Pattern &pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude,
                          int64_t amp_at, const double *fint, const double *a, const double *v, double alpha, double *out, hipStream_t s)
{
    k_tt_reactions<<<dim3((unsigned)((2 * pat.N + 255) / 256)), 256, 0, s>>>(pat, mval, known, f, amplitude, amp_at, fint, a, v, alpha, out);
}

// ---- an energy row: the kinetic energy and the load's work over the 2N DOFs, the strain energy over the elements (explicit_tl.h's
// tl_element_energy), each thread its fixed share of either
template <int LAW>
__global__ void __launch_bounds__(256) k_tt_energy_partials(TlMesh m, Pattern pat, const double *mval, const uint8_t *known, const double *u,
                                                            const double *v, const double *f, int32_t *inverted, double *partials)
{
    double acc[3] = {0.0, 0.0, 0.0};
    share_sum(2 * m.N, acc, [&](int64_t r, double (&s)[3]) {
        s[0] = fma(v[r], inertia_row(pat, mval, r, v, v, 0.0), s[0]);
        s[2] += known[r] ? 0.0 : f[r] * u[r];
    });
    share_sum(m.E, acc, [&](int64_t e, double (&s)[3]) { s[1] += tl_element_energy<LAW>(m, (const double2 *)u, e, inverted); });
    store_partials(acc, partials);
}

void tl_dynamic_energies(const TlMesh &m, const Pattern &pat, const double *mval, const uint8_t *known, const double *u, const double *v,
                         const double *f, const double *amplitude, int64_t amp_at, int32_t *inverted, double *partials, double *out,
                         hipStream_t s)
{
    (m.law == kLawNeoHooke ? k_tt_energy_partials<kLawNeoHooke> : k_tt_energy_partials<kLawSvk>)<<<dim3(kSensBlocks, 1), 256, 0, s>>>(
        m, pat, mval, known, u, v, f, inverted, partials);
    tl_row_sum(partials, amplitude, amp_at, out, s);
}

} // namespace magk
