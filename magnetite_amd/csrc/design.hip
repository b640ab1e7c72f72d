// The density design update (mag_design_init, mag_design_step) and the check of an element stiffness field
// (mag_set_element_scale), on the skeleton of member_pass.h: passes over elements, node passes on its node walk (sums in the
// order of the incidence lists), two-stage reductions of its fixed shape.  No floating-point atomics: a repeat gives the same
// bits.  Compiled -ffp-contract=off: the rounding is the source's, and tests/design_ref.py restates it line by line.
//
//   F x:     n_i = (sum_{e in i} a_e x_e) / A_i,  A_i = sum_{e in i} a_e;   (F x)_e = ((n_a + n_b) + n_c) / 3   (conn order)
//   F^T y:   m_i = sum_{e in i} y_e / 3;   (F^T y)_e = a_e ((m_a / A_a + m_b / A_b) + m_c / A_c)
//   OC:      Bq_e = max(-dJ/drho_e, 0) / w_e,   rho_new(L) = min(min(1, rho + move), max(max(rho_min, rho - move), rho sqrt(Bq / L))),
//            V(L) = sum_e w_e rho_new_e(L); min and max are fmin and fmax: where Bq / L is 0 / 0 the lower limit stands.
#include "design.h"
#include "member_pass.h"

namespace magk {

namespace {

// ---- node passes.  The node walk hands a pass the corners' fields; these passes read per-ELEMENT values instead, through the
// node's incidence list (entry k of it is the walk's k-th triangle), and ignore the one field they are given (the coordinates).
struct NodeSum {
    const uint32_t *inc;
    const int32_t *inc_off;
    struct Node {
        double sum;
        const uint32_t *list;
    };
    __device__ explicit NodeSum(const SensMesh &m) : inc(m.inc), inc_off(m.inc_off) {}
    __device__ Node node(int64_t pos) const { return {0.0, inc + inc_off[pos]}; }
};

struct NodeArea : NodeSum {
    const double *area;
    double *out;
    __device__ NodeArea(const SensMesh &m, const double *a, double *o) : NodeSum(m), area(a), out(o) {}
    __device__ void corner(Node &n, const double2 (&)[1][3], int32_t k) const { n.sum += area[n.list[k] / 3u]; }
    __device__ void store(const Node &n, int64_t at) const { out[at] = n.sum; }
};

// n_i of F
struct NodeAverage : NodeSum {
    const double *area, *node_area, *x;
    double *out;
    __device__ NodeAverage(const SensMesh &m, const double *a, const double *na, const double *x_, double *o)
        : NodeSum(m), area(a), node_area(na), x(x_), out(o)
    {
    }
    __device__ void corner(Node &n, const double2 (&)[1][3], int32_t k) const
    {
        const uint32_t e = n.list[k] / 3u;
        n.sum += area[e] * x[e];
    }
    __device__ void store(const Node &n, int64_t at) const { out[at] = n.sum / node_area[at]; } // (read by the node's elements only)
};

// m_i / A_i of F^T
struct NodeSpread : NodeSum {
    const double *node_area, *y;
    double *out;
    __device__ NodeSpread(const SensMesh &m, const double *na, const double *y_, double *o) : NodeSum(m), node_area(na), y(y_), out(o) {}
    __device__ void corner(Node &n, const double2 (&)[1][3], int32_t k) const { n.sum += y[n.list[k] / 3u] / 3.0; }
    __device__ void store(const Node &n, int64_t at) const { out[at] = n.sum / node_area[at]; }
};

template <class Pass, class... Args>
__global__ void __launch_bounds__(256) k_design_nodes(SensMesh mesh, const double2 *xy, Args... args)
{
    const double2 *const src[1] = {xy};
    gather_walk(mesh, src, Pass(mesh, args...));
}

// ---- reductions: two sums and two maxima (of values >= 0) per launch, member_pass.h's two stages.  partials: [kSensBlocks][2]
// sums, then [kSensBlocks][2] maxima.  Term: term(i, sums, maxima) per entry; Finish: finish(sums, maxima) in one thread.
template <class Term>
__global__ void __launch_bounds__(256) k_design_partials(int64_t n, Term term, double *partials)
{
    __shared__ double s_max[4 * 2];
    double acc[2] = {0.0, 0.0}, mx[2] = {0.0, 0.0};
    share_sum(n, acc, [&](int64_t i, double (&a)[2]) { term(i, a, mx); });
    store_partials(acc, partials);
    block_max256<2>(mx, s_max);
    if (threadIdx.x == 0) {
        double *out = partials + 2 * ((int64_t)kSensBlocks + blockIdx.x);
        out[0] = mx[0];
        out[1] = mx[1];
    }
}

template <class Finish>
__global__ void __launch_bounds__(256) k_design_finish(const double *partials, Finish finish)
{
    __shared__ double s_max[4 * 2];
    const double *in = partials + 2 * ((int64_t)kSensBlocks + threadIdx.x);
    double mx[2] = {in[0], in[1]};
    block_max256<2>(mx, s_max);
    sum_partials<2>(partials, [&](int64_t, const double (&acc)[2]) { finish(acc, mx); });
}

template <class Term, class Finish>
void reduce(int64_t n, const Term &term, const Finish &finish, double *partials, hipStream_t s)
{
    k_design_partials<<<dim3(kSensBlocks, 1), 256, 0, s>>>(n, term, partials);
    k_design_finish<<<dim3(1, 1), 256, 0, s>>>(partials, finish);
}

struct AreaTerm {
    const double *area;
    __device__ void operator()(int64_t e, double (&a)[2], double (&)[2]) const { a[0] += area[e]; }
};
struct AreaFinish {
    double *small, volume_fraction;
    __device__ void operator()(const double (&a)[2], const double (&)[2]) const
    {
        small[DW_AREA] = a[0];
        small[DW_TARGET] = volume_fraction * a[0];
    }
};

struct VolumeTerm {
    const double *rho, *w;
    __device__ void operator()(int64_t e, double (&a)[2], double (&)[2]) const { a[0] += w[e] * rho[e]; }
};
struct VolumeFinish {
    double *small;
    __device__ void operator()(const double (&a)[2], const double (&)[2]) const { small[DW_INFO + 0] = a[0] / small[DW_AREA]; }
};

struct GreyTerm {
    const double *rhof;
    __device__ void operator()(int64_t e, double (&a)[2], double (&)[2]) const { a[0] += 4.0 * rhof[e] * (1.0 - rhof[e]); }
};
struct GreyFinish {
    double *small, count;
    __device__ void operator()(const double (&a)[2], const double (&)[2]) const { small[DW_INFO + 3] = a[0] / count; }
};

struct BqTerm {
    const double *dJ_drho, *w;
    double *bq;
    __device__ void operator()(int64_t e, double (&)[2], double (&mx)[2]) const
    {
        const double b = fmax(-dJ_drho[e], 0.0) / w[e];
        bq[e] = b;
        mx[0] = fmax(mx[0], b);
    }
};
struct BqFinish {
    double *small, rho_min;
    __device__ void operator()(const double (&)[2], const double (&mx)[2]) const
    {
        small[DW_MAX_BQ] = mx[0];
        small[DW_LO] = 0.0;
        small[DW_HI] = mx[0] / (rho_min * rho_min);
    }
};

// V(L) at the bracket's midpoint (OC_MID: a bisection step; OC_APPLY: the step's result, rho_new written), at its lower or
// its upper end (OC_LO0, OC_HI0: asked once, while the bracket is the first one)
enum OcMode { OC_MID, OC_LO0, OC_HI0, OC_APPLY };

struct OcTerm {
    const double *rho, *bq, *w, *small;
    double *rho_new; // OC_APPLY
    double move, rho_min;
    int mode;
    __device__ void operator()(int64_t e, double (&a)[2], double (&mx)[2]) const
    {
        const double lo = small[DW_LO], hi = small[DW_HI];
        const double L = mode == OC_LO0 ? lo : (mode == OC_HI0 ? hi : 0.5 * (lo + hi));
        const double r = rho[e];
        const double next = fmin(fmin(1.0, r + move), fmax(fmax(rho_min, r - move), r * sqrt(bq[e] / L)));
        a[0] += w[e] * next;
        if (mode == OC_APPLY) {
            rho_new[e] = next;
            mx[0] = fmax(mx[0], fabs(next - r));
        }
    }
};
struct OcFinish {
    double *small;
    int mode;
    __device__ void operator()(const double (&a)[2], const double (&mx)[2]) const
    {
        const double V = a[0], mid = 0.5 * (small[DW_LO] + small[DW_HI]);
        if (mode == OC_MID) {
            if (V > small[DW_TARGET])
                small[DW_LO] = mid;
            else
                small[DW_HI] = mid;
        } else if (mode == OC_LO0) {
            small[DW_V_LO0] = V;
        } else if (mode == OC_HI0) {
            small[DW_V_HI0] = V;
        } else {
            small[DW_INFO + 0] = V / small[DW_AREA];
            small[DW_INFO + 1] = mid;
            small[DW_INFO + 2] = mx[0];
            small[DW_INFO + 4] = (small[DW_V_LO0] >= small[DW_TARGET] && small[DW_TARGET] >= small[DW_V_HI0]) ? 1.0 : 0.0;
        }
    }
};

// x^n, n >= 0, by repeated multiplication from the left
__device__ inline double ipow(double x, int n)
{
    if (n == 0) return 1.0;
    double p = x;
    for (int k = 1; k < n; ++k) p *= x;
    return p;
}

} // namespace

__global__ void __launch_bounds__(256) k_first_out_of_range(const double *x, int64_t n, double upper, int32_t *first)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    if (!(v > 0.0 && v <= upper && isfinite(v))) atomicMin(first, (int32_t)i);
}

__global__ void __launch_bounds__(256) k_design_areas(const int32_t *conn, const double2 *xy, int64_t E, double *area, int32_t *first)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const double2 c[3] = {xy[conn[3 * e]], xy[conn[3 * e + 1]], xy[conn[3 * e + 2]]};
    const double a = 0.5 * edges_of(c).A2;
    area[e] = a;
    if (!(a > 0.0 && isfinite(a))) atomicMin(first, (int32_t)e);
}

__global__ void __launch_bounds__(256) k_design_filter_elements(const int32_t *conn, int64_t E, const double *node, double *y)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    y[e] = ((node[conn[3 * e]] + node[conn[3 * e + 1]]) + node[conn[3 * e + 2]]) / 3.0;
}

__global__ void __launch_bounds__(256) k_design_filter_t_elements(const int32_t *conn, int64_t E, const double *area, const double *node,
                                                                  double *x)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    x[e] = area[e] * ((node[conn[3 * e]] + node[conn[3 * e + 1]]) + node[conn[3 * e + 2]]);
}

__global__ void __launch_bounds__(256) k_design_interpolate(const double *rhof, int64_t E, DesignParams p, double *scale)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    scale[e] = p.scale_min + (1.0 - p.scale_min) * ipow(rhof[e], p.penal);
}

__global__ void __launch_bounds__(256) k_design_chain(const double *dJ_ds, const double *energy, const double *scale, const double *rhof,
                                                      int64_t E, DesignParams p, double *dJ_drhof)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const double g = dJ_ds ? dJ_ds[e] : (-2.0 * energy[e]) / scale[e];
    dJ_drhof[e] = ((g * (1.0 - p.scale_min)) * (double)p.penal) * ipow(rhof[e], p.penal - 1);
}

static unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

void first_out_of_range(const double *x, int64_t n, double upper, int32_t *first, hipStream_t s)
{
    k_first_out_of_range<<<blocks_of(n), 256, 0, s>>>(x, n, upper, first);
}

void design_areas(const SensMesh &m, const double *xy, double *area, int32_t *first, hipStream_t s)
{
    k_design_areas<<<blocks_of(m.E), 256, 0, s>>>(m.conn, (const double2 *)xy, m.E, area, first);
}

void design_node_areas(const SensMesh &m, const double *xy, const double *area, double *node_area, hipStream_t s)
{
    k_design_nodes<NodeArea><<<dim3(blocks_of(m.N), 1), 256, 0, s>>>(m, (const double2 *)xy, area, node_area);
}

void design_total_area(const double *area, int64_t E, double volume_fraction, double *partials, double *small, hipStream_t s)
{
    reduce(E, AreaTerm{area}, AreaFinish{small, volume_fraction}, partials, s);
}

void design_filter(const SensMesh &m, const double *xy, const double *area, const double *node_area, const double *x, double *node,
                   double *y, hipStream_t s)
{
    k_design_nodes<NodeAverage><<<dim3(blocks_of(m.N), 1), 256, 0, s>>>(m, (const double2 *)xy, area, node_area, x, node);
    k_design_filter_elements<<<blocks_of(m.E), 256, 0, s>>>(m.conn, m.E, node, y);
}

void design_filter_t(const SensMesh &m, const double *xy, const double *area, const double *node_area, const double *y, double *node,
                     double *x, hipStream_t s)
{
    k_design_nodes<NodeSpread><<<dim3(blocks_of(m.N), 1), 256, 0, s>>>(m, (const double2 *)xy, node_area, y, node);
    k_design_filter_t_elements<<<blocks_of(m.E), 256, 0, s>>>(m.conn, m.E, area, node, x);
}

void design_interpolate(const double *rhof, int64_t E, const DesignParams &p, double *scale, hipStream_t s)
{
    k_design_interpolate<<<blocks_of(E), 256, 0, s>>>(rhof, E, p, scale);
}

void design_chain(const double *dJ_ds, const double *energy, const double *scale, const double *rhof, int64_t E, const DesignParams &p,
                  double *dJ_drhof, hipStream_t s)
{
    k_design_chain<<<blocks_of(E), 256, 0, s>>>(dJ_ds, energy, scale, rhof, E, p, dJ_drhof);
}

void design_oc(const double *rho, const double *dJ_drho, const double *w, int64_t E, const DesignParams &p, double *bq, double *rho_new,
               double *partials, double *small, hipStream_t s)
{
    reduce(E, BqTerm{dJ_drho, w, bq}, BqFinish{small, p.rho_min}, partials, s);
    const auto volume = [&](int mode) {
        reduce(E, OcTerm{rho, bq, w, small, rho_new, p.move, p.rho_min, mode}, OcFinish{small, mode}, partials, s);
    };
    volume(OC_LO0);
    volume(OC_HI0);
    for (int k = 0; k < kDesignBisections; ++k) volume(OC_MID);
    volume(OC_APPLY);
}

void design_volume(const double *rho, const double *w, int64_t E, double *partials, double *small, hipStream_t s)
{
    reduce(E, VolumeTerm{rho, w}, VolumeFinish{small}, partials, s);
}

void design_greyness(const double *rhof, int64_t E, double *partials, double *small, hipStream_t s)
{
    reduce(E, GreyTerm{rhof}, GreyFinish{small, (double)E}, partials, s);
}

} // namespace magk
