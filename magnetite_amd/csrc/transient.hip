// Transient dynamics (mag_run_transient): the device side of Newmark's method on the uploaded part -- the mass in K's block-CSR
// pattern, the effective matrix, the pattern's operator y = K x1 + M x2, the fused vector updates and the records.  The method is
// stated in transient.h.  Compiled -ffp-contract=off: the rounding is the source's; no floating-point atomics and every sum in a
// fixed order: a repeat gives the same bits, and a resumed run the bits of the run it continues.
#include "transient.h"
#include "member_pass.h"

namespace magk {

// ---- the mass in the pattern: one thread per row node (Hilbert position g, caller id perm[g]); the row's scalars are zeroed,
// then every incident triangle adds to the three blocks of its corners, in list order
__global__ void __launch_bounds__(256) k_tr_mass_pattern(Pattern pat, const uint32_t *perm, const int32_t *inc_off, const uint32_t *inc,
                                                         const int32_t *conn, const double2 *xy, double c, int32_t lumped, double *mval)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= pat.N) return;
    const int64_t i = perm[g];
    const int32_t p = pat.bptr[i], cnt = pat.bptr[i + 1] - p;
    for (int32_t k = 0; k < cnt; ++k) mval[p + k] = 0.0;
    const int32_t q1 = inc_off[g + 1];
    for (int32_t q = inc_off[g]; q < q1; ++q) {
        const uint32_t w = inc[q];
        const int64_t e = w / 3u;
        const int a = (int)(w - 3u * (uint32_t)e);
        const int32_t nn[3] = {conn[3 * e], conn[3 * e + 1], conn[3 * e + 2]};
        const double2 cs[3] = {xy[nn[0]], xy[nn[1]], xy[nn[2]]};
        const double me = c * (0.5 * fabs(edges_of(cs).A2));
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            if (lumped && b != a) continue;
            const double w_b = lumped ? me / 3.0 : (b == a ? me / 6.0 : me / 12.0);
            const int32_t j = b == 0 ? nn[0] : (b == 1 ? nn[1] : nn[2]);
            for (int32_t k = 0; k < cnt; ++k) // (the column is one of the row's: K couples the same pairs)
                if (pat.bcol[p + k] == j) {
                    mval[p + k] = mval[p + k] + w_b;
                    break;
                }
        }
    }
}

void mass_pattern(const Pattern &pat, const uint32_t *perm, const int32_t *inc_off, const uint32_t *inc, const int32_t *conn,
                  const double *xy, double c, int32_t lumped, double *mval, hipStream_t s)
{
    k_tr_mass_pattern<<<dim3((unsigned)((pat.N + 255) / 256)), 256, 0, s>>>(pat, perm, inc_off, inc, conn, (const double2 *)xy, c, lumped, mval);
}

// ---- A = c_K K + c_M M: one thread per scalar row r = 2 i + d; the mass sits on entry d of each of the row's pairs
__global__ void __launch_bounds__(256) k_tr_effective(Pattern pat, const double *kval, const double *mval, double c_K, double c_M, double *aval)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= 2 * pat.N) return;
    const int64_t i = r >> 1;
    const int d = (int)(r & 1);
    const int32_t p = pat.bptr[i], cnt = pat.bptr[i + 1] - p;
    const int64_t at = 4 * (int64_t)p + (int64_t)d * 2 * cnt;
    for (int32_t k = 0; k < cnt; ++k) {
        const double m = c_M * mval[p + k];
        const double k0 = c_K * kval[at + 2 * k], k1 = c_K * kval[at + 2 * k + 1];
        aval[at + 2 * k] = d == 0 ? k0 + m : k0;
        aval[at + 2 * k + 1] = d == 1 ? k1 + m : k1;
    }
}

void effective_values(const Pattern &pat, const double *kval, const double *mval, double c_K, double c_M, double *aval, hipStream_t s)
{
    k_tr_effective<<<dim3((unsigned)((2 * pat.N + 255) / 256)), 256, 0, s>>>(pat, kval, mval, c_K, c_M, aval);
}

// ---- y = K x1 + M x2 over the block rows
__global__ void __launch_bounds__(256) k_tr_pattern_apply(Pattern pat, PatternApply a)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= 2 * pat.N) return;
    const int64_t i = r >> 1;
    const int d = (int)(r & 1);
    const int32_t p = pat.bptr[i], cnt = pat.bptr[i + 1] - p;
    const double *row = a.kval + 4 * (int64_t)p + (int64_t)d * 2 * cnt;
    const bool k_on = a.xa || a.xb, m_on = a.xc || a.xd;
    double sk = 0.0, sm = 0.0, su = 0.0, sv = 0.0;
    for (int32_t k = 0; k < cnt; ++k) {
        const int64_t j = pat.bcol[p + k];
        if (k_on) { // (the same for every thread of the launch, like the tests of the pointers below)
            double x0 = 0.0, x1 = 0.0;
            if (a.xa) x0 = a.ca * a.xa[2 * j], x1 = a.ca * a.xa[2 * j + 1];
            if (a.xb) x0 = x0 + a.cb * a.xb[2 * j], x1 = x1 + a.cb * a.xb[2 * j + 1];
            sk += row[2 * k] * x0;
            sk += row[2 * k + 1] * x1;
        }
        if (m_on) {
            double x = 0.0;
            if (a.xc) x = a.cc * a.xc[2 * j + d];
            if (a.xd) x = x + a.cd * a.xd[2 * j + d];
            sm += a.mval[p + k] * x;
        }
        if (a.ku) {
            su += row[2 * k] * a.xa[2 * j];
            su += row[2 * k + 1] * a.xa[2 * j + 1];
        }
        if (a.mv) sv += a.mval[p + k] * a.xc[2 * j + d];
    }
    const double y = sk + sm;
    if (a.kind == 0) {
        a.y[r] = y;
    } else {
        const double load = a.amplitude[a.amp_at] * a.f[r];
        const bool known = a.known[r] != 0;
        a.y[r] = a.kind == 1 ? (known ? 0.0 : load - y) : (known ? y : load);
    }
    if (a.ku) a.ku[r] = su;
    if (a.mv) a.mv[r] = sv;
}

void pattern_apply(const Pattern &pat, const PatternApply &a, hipStream_t s)
{
    k_tr_pattern_apply<<<dim3((unsigned)((2 * pat.N + 255) / 256)), 256, 0, s>>>(pat, a);
}

// ---- the vector updates.  The records of a step are written by threads of their own (behind the 2N of the update), which
// redo the update of their DOF from the same inputs: the same bits, and no thread waits for another
__global__ void __launch_bounds__(256) k_tr_predict(NewmarkState st, double c_uv, double c_ua, double c_va)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= st.n2) return;
    if (st.known[d]) {
        st.ut[d] = st.u_in[d];
        st.vt[d] = 0.0;
        return;
    }
    const double u = st.u[d], v = st.v[d], a = st.a[d];
    st.ut[d] = (u + c_uv * v) + c_ua * a;
    st.vt[d] = v + c_va * a;
}

void newmark_predict(const NewmarkState &st, double dt, double beta, double gamma, hipStream_t s)
{
    k_tr_predict<<<dim3((unsigned)((st.n2 + 255) / 256)), 256, 0, s>>>(st, dt, dt * dt * (0.5 - beta), dt * (1.0 - gamma));
}

__global__ void __launch_bounds__(256) k_tr_correct(NewmarkState st, double c_u, double c_v, int64_t row, double *snap)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool probe = t >= st.n2;
    if (probe && t - st.n2 >= st.num_probes) return;
    const int64_t d = probe ? st.probes[t - st.n2] : t;
    const double a = st.a[d];
    const double u = st.ut[d] + c_u * a, v = st.vt[d] + c_v * a;
    if (probe) {
        const int64_t at = row * st.num_probes + (t - st.n2);
        st.probe_u[at] = u;
        st.probe_v[at] = v;
        st.probe_a[at] = a;
        return;
    }
    st.u[d] = u;
    st.v[d] = v;
    if (snap) snap[d] = u;
}

void newmark_correct(const NewmarkState &st, double dt, double beta, double gamma, int64_t row, double *snap, hipStream_t s)
{
    k_tr_correct<<<dim3((unsigned)((st.n2 + st.num_probes + 255) / 256)), 256, 0, s>>>(st, beta * dt * dt, gamma * dt, row, snap);
}

__global__ void __launch_bounds__(256) k_tr_record(NewmarkState st, int64_t row, double *snap)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool probe = t >= st.n2;
    if (probe && t - st.n2 >= st.num_probes) return;
    if (probe) {
        const int64_t d = st.probes[t - st.n2], at = row * st.num_probes + (t - st.n2);
        st.probe_u[at] = st.u[d];
        st.probe_v[at] = st.v[d];
        st.probe_a[at] = st.a[d];
    } else if (snap) {
        snap[t] = st.u[t];
    }
}

void newmark_record(const NewmarkState &st, int64_t row, double *snap, hipStream_t s)
{
    k_tr_record<<<dim3((unsigned)((st.n2 + st.num_probes + 255) / 256)), 256, 0, s>>>(st, row, snap);
}

__global__ void __launch_bounds__(256) k_tr_start(NewmarkState st, const double *u0, const double *v0)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= st.n2) return;
    const bool known = st.known[d] != 0;
    st.u[d] = known ? st.u_in[d] : (u0 ? u0[d] : 0.0);
    st.v[d] = known ? 0.0 : (v0 ? v0[d] : 0.0);
    st.a[d] = 0.0;
}

void newmark_start(const NewmarkState &st, const double *u0, const double *v0, hipStream_t s)
{
    k_tr_start<<<dim3((unsigned)((st.n2 + 255) / 256)), 256, 0, s>>>(st, u0, v0);
}

// ---- the energies, the two stages
__global__ void __launch_bounds__(256) k_tr_energy_partials(NewmarkState st, const double *ku, const double *mv, const double *f, double *partials)
{
    double acc[3] = {0.0, 0.0, 0.0};
    share_sum(st.n2, acc, [=](int64_t i, double (&a)[3]) {
        a[0] += st.v[i] * mv[i];
        a[1] += st.u[i] * ku[i];
        a[2] += st.known[i] ? 0.0 : f[i] * st.u[i];
    });
    store_partials(acc, partials);
}

__global__ void __launch_bounds__(256) k_tr_energy_sum(const double *partials, const double *amplitude, int64_t amp_at, double *out)
{
    sum_partials<3>(partials, [&](int64_t, const double (&acc)[3]) {
        out[0] = 0.5 * acc[0];
        out[1] = 0.5 * acc[1];
        out[2] = amplitude[amp_at] * acc[2];
    });
}

void newmark_energies(const NewmarkState &st, const double *ku, const double *mv, const double *f, const double *amplitude,
                      int64_t amp_at, double *partials, double *out, hipStream_t s)
{
    k_tr_energy_partials<<<dim3(kSensBlocks, 1), 256, 0, s>>>(st, ku, mv, f, partials);
    k_tr_energy_sum<<<dim3(1, 1), 256, 0, s>>>(partials, amplitude, amp_at, out);
}

// ---- a caller-numbered vector in the compact numbering of the free DOFs
__global__ void __launch_bounds__(256) k_tr_compact(const double *x, const int32_t *fidx, const uint8_t *known, int64_t n2, double *b)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d < n2 && !known[d]) b[fidx[d]] = x[d];
}

void compact_free(const double *x, const int32_t *fidx, const uint8_t *known, int64_t n2, double *b, hipStream_t s)
{
    k_tr_compact<<<dim3((unsigned)((n2 + 255) / 256)), 256, 0, s>>>(x, fidx, known, n2, b);
}

// ---- the first probe out of range, by an (integer) minimum over offenders only
__global__ void __launch_bounds__(256) k_tr_check_probes(const int32_t *probes, int32_t num_probes, int64_t n2, unsigned long long *bad)
{
    const int32_t k = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (k >= num_probes) return;
    if (probes[k] < 0 || probes[k] >= n2) atomicMin(bad, (unsigned long long)k);
}

void check_probes(const int32_t *probes, int32_t num_probes, int64_t n2, unsigned long long *bad, hipStream_t s)
{
    (void)hipMemsetAsync(bad, 0xff, 8, s);
    if (num_probes > 0) k_tr_check_probes<<<dim3((unsigned)((num_probes + 255) / 256)), 256, 0, s>>>(probes, num_probes, n2, bad);
}

} // namespace magk
