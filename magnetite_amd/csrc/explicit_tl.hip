// Explicit dynamics with large rotations (mag_run_explicit with kinematics = MAG_KIN_TOTAL_LAGRANGIAN, mag_internal_force): the
// total-Lagrangian internal force f_int(u) of explicit_tl.h in place of K u.  A whole time step is one launch of
// k_explicit_tl_step, which reads no matrix: k_explicit_step's skeleton (explicit.hip) around k_operator_lds's ring walk (cg.hip)
// with fan_force_tl as the triangle's function.  Compiled -ffp-contract=off: the rounding is the source's; no floating-point
// atomics, every sum in a fixed order (a node's in its ring's, or its incidence list's): a repeat gives the same bits, every grid
// gives the same bits, and a resumed run the bits of the run it continues.  The ring's order depends on the tile size, so the bits
// may differ across tile_nodes (the linear step's do not: its row order is the table's).
#include "explicit_tl.h"
#include "member_pass.h"

namespace magk {

constexpr int kTlSlotRegs = 5; // ring words kept in registers, as cg.hip's kSlotRegs: 10 entries, a closed fan of valence <= 9

// Persistent over tiles, one lane per owned node.  A launch reads P.f.in and writes P.f.out, so a tile never sees a neighbour's new
// state; a halo node's predictor is recomputed from the same inputs as its owner's: the same bits.  LDS: cap * 32 bytes (the
// images of the reference coordinates and of ut).
template <int B, int LAW>
__global__ void __launch_bounds__(B) k_explicit_tl_step(const ExplicitTlParams P)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_tl[];
    const StepFrame &F = P.f;
    double2 *s_xy = s_tl, *s_u = s_tl + F.cap;
    const int tid = threadIdx.x;
    const double dt = F.dt;
    const StepCoef c = step_coef(F);
    const double c0 = P.c0, nu = P.nu, h = P.h;
    int32_t *inverted = P.inverted;

    for (int32_t t = blockIdx.x; t < F.T; t += gridDim.x) {
        const int64_t node = (int64_t)t * B + tid;
        const bool valid = node < F.N;
        const int32_t deg = P.tile_deg[t], hoff = P.tile_hoff[t], nh = P.tile_hoff[t + 1] - hoff;
        const uint32_t *ell = P.ell16 + P.tile_off[t] + tid;
        uint32_t w[kTlSlotRegs];
#pragma unroll
        for (int k = 0; k < kTlSlotRegs; ++k) w[k] = k < deg ? ell[(int64_t)k * B] : 0xffffffffu;

        uint8_t m = 3;
        double2 ca = make_double2(0.0, 0.0), ut = ca, vt = ca, fl = ca;
        double mass = 1.0;
        if (valid) {
            const ExRec r = F.in[node];
            m = F.maskP[node];
            explicit_predict(r, m, F.uinP[node], dt, c.c_ua, c.c_va, ut, vt);
            fl = F.fP[node];
            mass = F.massP[node];
            ca = P.xyP[node];
        }
        __syncthreads(); // the previous tile's readers are done with the images
        s_xy[tid] = ca;
        s_u[tid] = ut;
        for (int32_t hh = tid; hh < nh; hh += B) { // (more halo nodes than threads: rare)
            const int32_t hg = F.halo_g[hoff + hh];
            s_xy[B + hh] = P.halo_xy[hoff + hh]; // the static per-tile copy: coalesced, independent of the index load
            double2 hut, hvt; // (the velocity is not used: the force reads ut alone)
            explicit_predict(F.in[hg], F.maskP[hg], F.uinP[hg], dt, c.c_ua, c.c_va, hut, hvt);
            s_u[B + hh] = hut;
        }
        __syncthreads();

        double fx = 0.0, fy = 0.0;
        {
            double2 rd = ca, ru = ut; // the previous ring entry, relative to this node; every fan starts with the break bit
            auto tri = [&](const double2 db, const double2 ub, const double2 dc, const double2 uc) {
                fan_force_tl<LAW>(db, ub, dc, uc, c0, nu, h, fx, fy, inverted);
            };
#pragma unroll
            for (int k = 0; k < kTlSlotRegs; ++k) ring_word(w[k], s_xy, s_u, ca, ut, rd, ru, tri);
            for (int32_t k = kTlSlotRegs; k < deg; ++k) ring_word(ell[(int64_t)k * B], s_xy, s_u, ca, ut, rd, ru, tri);
        }

        if (valid) explicit_correct(F, c, node, m, ut, vt, fl, mass, fx, fy);
    }
}

static size_t explicit_tl_lds(int32_t cap) { return (size_t)cap * 32; }

typedef void (*explicit_tl_fn)(const ExplicitTlParams);
template <int LAW>
static explicit_tl_fn explicit_tl_pick_b(int32_t B)
{
    return B == 256 ? k_explicit_tl_step<256, LAW> : (B == 1024 ? k_explicit_tl_step<1024, LAW> : k_explicit_tl_step<512, LAW>);
}
static explicit_tl_fn explicit_tl_pick(int32_t B, int32_t law)
{
    return law == kLawNeoHooke ? explicit_tl_pick_b<kLawNeoHooke>(B) : explicit_tl_pick_b<kLawSvk>(B);
}

int explicit_tl_grid(int32_t B, int32_t cap, int32_t tiles, int32_t law)
{
    return step_grid((const void *)explicit_tl_pick(B, law), step_threads(B), explicit_tl_lds(cap), tiles);
}

void explicit_tl_step(const ExplicitTlParams &P, int32_t B, int32_t grid, hipStream_t s)
{
    explicit_tl_pick(B, P.law)<<<grid, step_threads(B), explicit_tl_lds(P.f.cap), s>>>(P);
}

// ---- f_int(u) in caller numbering: lane g takes the node at Hilbert position g and fetches every corner through conn.
// inc[k] = 3e + (the corner of e that is this node); the triangle is taken from that corner on, counter-clockwise
template <int LAW>
__global__ void __launch_bounds__(256) k_tl_force(TlMesh m, const double2 *u, double2 *f, int32_t *inverted)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= m.N) return;
    const int64_t i = m.perm[g];
    const double2 ca = m.xy[i], ua = u[i];
    double fx = 0.0, fy = 0.0;
    const int32_t q1 = m.inc_off[g + 1];
    for (int32_t q = m.inc_off[g]; q < q1; ++q) {
        const uint32_t w = m.inc[q];
        const int64_t e = w / 3u;
        const int a = (int)(w - 3u * (uint32_t)e);
        const int64_t b = m.conn[3 * e + (a + 1) % 3], c = m.conn[3 * e + (a + 2) % 3];
        const double2 cb = m.xy[b], cc = m.xy[c], pb = u[b], pc = u[c];
        fan_force_tl<LAW>(make_double2(cb.x - ca.x, cb.y - ca.y), make_double2(pb.x - ua.x, pb.y - ua.y), make_double2(cc.x - ca.x, cc.y - ca.y),
                          make_double2(pc.x - ua.x, pc.y - ua.y), m.c0, m.nu, m.h, fx, fy, inverted);
    }
    f[i] = make_double2(fx, fy);
}

// ---- W(u): stage one over the elements, stage two over the kSensBlocks partial records
template <int LAW>
__global__ void __launch_bounds__(256) k_tl_energy_partials(TlMesh m, const double2 *u, int32_t *inverted, double *partials)
{
    double acc[1] = {0.0};
    share_sum(m.E, acc, [&](int64_t e, double (&a)[1]) { a[0] += tl_element_energy<LAW>(m, u, e, inverted); });
    store_partials(acc, partials);
}

__global__ void __launch_bounds__(256) k_tl_energy_sum(const double *partials, double *out)
{
    sum_partials<1>(partials, [&](int64_t, const double (&acc)[1]) { out[0] = acc[0]; });
}

void tl_force(const TlMesh &m, const double *u, double *f, int32_t *inverted, double *partials, double *energy, hipStream_t s)
{
    const bool neo = m.law == kLawNeoHooke;
    (neo ? k_tl_force<kLawNeoHooke> : k_tl_force<kLawSvk>)<<<dim3((unsigned)((m.N + 255) / 256)), 256, 0, s>>>(m, (const double2 *)u, (double2 *)f,
                                                                                                      inverted);
    if (!energy) return;
    (neo ? k_tl_energy_partials<kLawNeoHooke> : k_tl_energy_partials<kLawSvk>)<<<dim3(kSensBlocks, 1), 256, 0, s>>>(m, (const double2 *)u, inverted,
                                                                                                                partials);
    k_tl_energy_sum<<<dim3(1, 1), 256, 0, s>>>(partials, energy);
}

// ---- the unfused step's subtraction and division by the mass: one thread per DOF
__global__ void __launch_bounds__(256) k_tl_divide(Pattern pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude,
                                                   int64_t amp_at, const double *fint, const double *vt, double alpha, double c, double *a)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= 2 * pat.N) return;
    const double m = diagonal_mass(pat, mval, r >> 1);
    a[r] = known[r] ? 0.0 : (amplitude[amp_at] * f[r] - (fint[r] + m * (alpha * vt[r]))) / (c * m);
}

void tl_divide(const Pattern &pat, const double *mval, const uint8_t *known, const double *f, const double *amplitude, int64_t amp_at,
               const double *fint, const double *vt, double alpha, double c, double *a, hipStream_t s)
{
    k_tl_divide<<<dim3((unsigned)((2 * pat.N + 255) / 256)), 256, 0, s>>>(pat, mval, known, f, amplitude, amp_at, fint, vt, alpha, c, a);
}

__global__ void __launch_bounds__(256) k_tl_reactions(const uint8_t *known, const double *f, const double *amplitude, int64_t amp_at,
                                                      const double *fint, int64_t n2, double *out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n2) return;
    out[r] = known[r] ? fint[r] : amplitude[amp_at] * f[r];
}

void tl_reactions(const uint8_t *known, const double *f, const double *amplitude, int64_t amp_at, const double *fint, int64_t n2, double *out,
                  hipStream_t s)
{
    k_tl_reactions<<<dim3((unsigned)((n2 + 255) / 256)), 256, 0, s>>>(known, f, amplitude, amp_at, fint, n2, out);
}

// ---- an energy row: the kinetic energy and the load's work over the 2N DOFs, the strain energy over the elements, each thread
// its fixed share of either
template <int LAW>
__global__ void __launch_bounds__(256) k_tl_row_partials(TlMesh m, Pattern pat, const double *mval, const uint8_t *known, const double *u,
                                                         const double *v, const double *f, int32_t *inverted, double *partials)
{
    double acc[3] = {0.0, 0.0, 0.0};
    share_sum(2 * m.N, acc, [&](int64_t r, double (&a)[3]) {
        const double mm = diagonal_mass(pat, mval, r >> 1);
        a[0] += v[r] * (mm * v[r]);
        a[2] += known[r] ? 0.0 : f[r] * u[r];
    });
    share_sum(m.E, acc, [&](int64_t e, double (&a)[3]) { a[1] += tl_element_energy<LAW>(m, (const double2 *)u, e, inverted); });
    store_partials(acc, partials);
}

__global__ void __launch_bounds__(256) k_tl_row_sum(const double *partials, const double *amplitude, int64_t amp_at, double *out)
{
    sum_partials<3>(partials, [&](int64_t, const double (&acc)[3]) {
        out[0] = 0.5 * acc[0];
        out[1] = acc[1];
        out[2] = amplitude[amp_at] * acc[2];
    });
}

void tl_row_sum(const double *partials, const double *amplitude, int64_t amp_at, double *out, hipStream_t s)
{
    k_tl_row_sum<<<dim3(1, 1), 256, 0, s>>>(partials, amplitude, amp_at, out);
}

void tl_energies(const TlMesh &m, const Pattern &pat, const double *mval, const uint8_t *known, const double *u, const double *v, const double *f,
                 const double *amplitude, int64_t amp_at, int32_t *inverted, double *partials, double *out, hipStream_t s)
{
    (m.law == kLawNeoHooke ? k_tl_row_partials<kLawNeoHooke> : k_tl_row_partials<kLawSvk>)<<<dim3(kSensBlocks, 1), 256, 0, s>>>(
        m, pat, mval, known, u, v, f, inverted, partials);
    tl_row_sum(partials, amplitude, amp_at, out, s);
}

} // namespace magk
