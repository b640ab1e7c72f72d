// Explicit dynamics (mag_run_explicit): central differences on the lumped mass.  A whole time step is one launch of
// k_explicit_step over the tile-local block rows of the assembled K (symbolic.hip, k_field_rows; gathered unmasked by cg.hip's
// k_field_gather); the method is stated in explicit.h.  Compiled -ffp-contract=off: the rounding is the source's (the row
// product's multiply-adds are written as the fma() they are); no floating-point atomics, every sum in a fixed order, and the row
// order is the table's -- the diagonal block, then ascending Hilbert index -- whatever the tile size: the same bits for every
// tile_nodes and every grid, a repeat gives the same bits, and a resumed run the bits of the run it continues.
#include "explicit.h"
#include "member_pass.h"

#include <cstdlib>

namespace magk {

// slots of the first entries of a row, loaded ahead of the values (k_cg_field's kFieldSlotRegs)
template <int B>
constexpr int kExplicitSlotRegs = B == 1024 ? 4 : 8;

// k_cg_field's skeleton without the dot products, the FusedState and the preconditioner: persistent over tiles, one lane per
// owned node.  A launch reads P.f.in and writes P.f.out, so a tile never sees a neighbour's new state; a halo node's predictors are
// recomputed from the same inputs as its owner's: the same bits.  LDS: cap * 16 bytes (the image of w = ut + eta vt).
template <int B>
__global__ void __launch_bounds__(B) k_explicit_step(const ExplicitParams P)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_w[];
    const int tid = threadIdx.x;
    const StepFrame &F = P.f;
    const double dt = F.dt, eta = P.eta;
    const StepCoef c = step_coef(F);
    constexpr int SR = kExplicitSlotRegs<B>;

    for (int32_t t = blockIdx.x; t < F.T; t += gridDim.x) {
        const FieldTileMeta tm = P.meta[t];
        const int64_t node = (int64_t)t * B + tid;
        const bool valid = node < F.N;
        const int32_t width = tm.width, nh = tm.nh, hoff = tm.hoff;
        const uint16_t *sl = P.slot + tm.off + tid;
        const double2 *v0 = P.fval + tm.off + tid, *v1 = v0 + P.total;
        uint32_t w[SR];
#pragma unroll
        for (int k = 0; k < SR; ++k) w[k] = k < width ? sl[(int64_t)k * B] : (uint32_t)tid;

        uint8_t m = 3;
        double2 ut = make_double2(0.0, 0.0), vt = ut, fl = ut;
        double mass = 1.0;
        if (valid) {
            m = F.maskP[node];
            explicit_predict(F.in[node], m, F.uinP[node], dt, c.c_ua, c.c_va, ut, vt);
            fl = F.fP[node];
            mass = F.massP[node];
        }
        __syncthreads(); // the previous tile's readers are done with the image
        s_w[tid] = make_double2(ut.x + eta * vt.x, ut.y + eta * vt.y);
        for (int32_t hh = tid; hh < nh; hh += B) { // (more halo nodes than threads: rare)
            const int32_t hg = F.halo_g[hoff + hh];
            double2 hut, hvt;
            explicit_predict(F.in[hg], F.maskP[hg], F.uinP[hg], dt, c.c_ua, c.c_va, hut, hvt);
            s_w[B + hh] = make_double2(hut.x + eta * hvt.x, hut.y + eta * hvt.y);
        }
        __syncthreads();

        double kx = 0.0, ky = 0.0;
        auto entry = [&](const uint32_t s, const int64_t k) {
            const double2 a0 = v0[k * B], a1 = v1[k * B];
            const double2 wv = s_w[s];
            kx = fma(a0.y, wv.y, fma(a0.x, wv.x, kx));
            ky = fma(a1.y, wv.y, fma(a1.x, wv.x, ky));
        };
#pragma unroll
        for (int k = 0; k < SR; ++k)
            if (k < width) entry(w[k], k);
#pragma unroll 2
        for (int32_t k = SR; k < width; ++k) entry(sl[(int64_t)k * B], k);

        if (valid) explicit_correct(F, c, node, m, ut, vt, fl, mass, kx, ky);
    }
}

static size_t explicit_lds(int32_t cap) { return (size_t)cap * 16; }

typedef void (*explicit_fn)(const ExplicitParams);
static explicit_fn explicit_pick(int32_t B) { return B == 256 ? k_explicit_step<256> : (B == 1024 ? k_explicit_step<1024> : k_explicit_step<512>); }

int step_grid(const void *kernel, int threads, size_t lds, int32_t tiles)
{
    int dev = 0, cus = 256, per_cu = 1;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    long g = (long)per_cu * cus;
    if (const char *cap_env = getenv("MAG_TUNE_GRID"))
        if (atoi(cap_env) > 0 && g > atoi(cap_env)) g = atoi(cap_env);
    if (g > tiles) g = tiles;
    return g < 1 ? 1 : (int)g;
}

int explicit_grid(int32_t B, int32_t cap, int32_t tiles) { return step_grid((const void *)explicit_pick(B), step_threads(B), explicit_lds(cap), tiles); }

void explicit_step(const ExplicitParams &P, int32_t B, int32_t grid, hipStream_t s)
{
    explicit_pick(B)<<<grid, step_threads(B), explicit_lds(P.f.cap), s>>>(P);
}

// ---- the inputs in Hilbert order: one thread per node
__global__ void __launch_bounds__(256) k_ex_inputs(Pattern pat, const uint32_t *perm, const double *mval, const double2 *u_in, const double2 *f_in,
                                                   double *massP, double2 *uinP, double2 *fP)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= pat.N) return;
    const int64_t i = perm[g];
    massP[g] = diagonal_mass(pat, mval, i);
    uinP[g] = u_in[i];
    fP[g] = f_in[i];
}

void explicit_inputs(const Pattern &pat, const uint32_t *perm, const double *mval, const double *u_in, const double *f_in, double *massP,
                     double2 *uinP, double2 *fP, hipStream_t s)
{
    k_ex_inputs<<<dim3((unsigned)((pat.N + 255) / 256)), 256, 0, s>>>(pat, perm, mval, (const double2 *)u_in, (const double2 *)f_in, massP, uinP, fP);
}

__global__ void __launch_bounds__(256) k_ex_gather(const uint32_t *perm, int64_t N, const double2 *u, const double2 *v, const double2 *a, ExRec *rec)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    const int64_t i = perm[g];
    ExRec r;
    r.u = u[i];
    r.v = v[i];
    r.a = a[i];
    rec[g] = r;
}

void explicit_gather(const uint32_t *perm, int64_t N, const double *u, const double *v, const double *a, ExRec *rec, hipStream_t s)
{
    k_ex_gather<<<dim3((unsigned)((N + 255) / 256)), 256, 0, s>>>(perm, N, (const double2 *)u, (const double2 *)v, (const double2 *)a, rec);
}

__global__ void __launch_bounds__(256) k_ex_scatter(const uint32_t *perm, int64_t N, const ExRec *rec, double2 *u, double2 *v, double2 *a)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    const int64_t i = perm[g];
    const ExRec r = rec[g];
    u[i] = r.u;
    v[i] = r.v;
    a[i] = r.a;
}

void explicit_scatter(const uint32_t *perm, int64_t N, const ExRec *rec, double *u, double *v, double *a, hipStream_t s)
{
    k_ex_scatter<<<dim3((unsigned)((N + 255) / 256)), 256, 0, s>>>(perm, N, rec, (double2 *)u, (double2 *)v, (double2 *)a);
}

// ---- the bound: stage one over the 2N rows of the pattern (a row's sum in ascending column order), stage two over the
// kSensBlocks partial records; a maximum and a minimum: the order does not matter, the shape is fixed all the same.
// Record: (the largest ratio, minus the smallest node mass)
__global__ void __launch_bounds__(256) k_ex_bound_partials(Pattern pat, const double *kval, const double *mval, const uint8_t *known, double *partials)
{
    __shared__ double s_red[8];
    double acc[2] = {0.0, -INFINITY};
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < 2 * pat.N; r += (int64_t)kSensBlocks * 256) {
        const int64_t i = r >> 1;
        const int d = (int)(r & 1);
        const int32_t p = pat.bptr[i], cnt = pat.bptr[i + 1] - p;
        const double *row = kval + 4 * (int64_t)p + (int64_t)d * 2 * cnt;
        double sum = 0.0, m = 0.0;
        for (int32_t k = 0; k < cnt; ++k) {
            const int64_t j = pat.bcol[p + k];
            if (j == i) m = mval[p + k];
            if (!known[2 * j]) sum += fabs(row[2 * k]);
            if (!known[2 * j + 1]) sum += fabs(row[2 * k + 1]);
        }
        if (!known[r]) acc[0] = fmax(acc[0], sum / m);
        if (d == 0) acc[1] = fmax(acc[1], -m);
    }
    block_max256<2>(acc, s_red);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = acc[0];
        partials[2 * blockIdx.x + 1] = acc[1];
    }
}

__global__ void __launch_bounds__(256) k_ex_bound_max(const double *partials, double *out)
{
    static_assert(kSensBlocks == 256, "one partial record per thread");
    __shared__ double s_red[8];
    double acc[2] = {partials[2 * threadIdx.x], partials[2 * threadIdx.x + 1]};
    block_max256<2>(acc, s_red);
    if (threadIdx.x == 0) {
        out[0] = acc[0];
        out[1] = -acc[1];
    }
}

void explicit_bound(const Pattern &pat, const double *kval, const double *mval, const uint8_t *known, double *partials, double *out,
                    hipStream_t s)
{
    k_ex_bound_partials<<<dim3(kSensBlocks), 256, 0, s>>>(pat, kval, mval, known, partials);
    k_ex_bound_max<<<dim3(1), 256, 0, s>>>(partials, out);
}

// ---- the unfused step's division by the mass: one thread per DOF
__global__ void __launch_bounds__(256) k_ex_divide(Pattern pat, const double *mval, const uint8_t *known, const double *rhs, double c, double *a)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= 2 * pat.N) return;
    const double m = diagonal_mass(pat, mval, r >> 1);
    a[r] = known[r] ? 0.0 : rhs[r] / (c * m);
}

void explicit_divide(const Pattern &pat, const double *mval, const uint8_t *known, const double *rhs, double c, double *a, hipStream_t s)
{
    k_ex_divide<<<dim3((unsigned)((2 * pat.N + 255) / 256)), 256, 0, s>>>(pat, mval, known, rhs, c, a);
}

__global__ void __launch_bounds__(256) k_ex_finite(const double *u, const double *v, const double *a, int64_t n2, int32_t *flag)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n2) return;
    if (!(isfinite(u[d]) && isfinite(v[d]) && isfinite(a[d]))) atomicOr(flag, 1);
}

void explicit_finite(const double *u, const double *v, const double *a, int64_t n2, int32_t *flag, hipStream_t s)
{
    k_ex_finite<<<dim3((unsigned)((n2 + 255) / 256)), 256, 0, s>>>(u, v, a, n2, flag);
}

} // namespace magk
