// magnetite_solver.hpp -- C++ host-side mirror of Magnetite's solver interface over the C ABI
// (include/magnetite_hip.h).  Header-only; link with -lmagnetite_hip.
//
// The reference is compiled Rust and this image has no Rust toolchain, so the host side above the C ABI is
// written in C++ with the reference's own names, argument meaning and error behaviour:
//   datatypes.rs:1-29   Vertex, Node, Element, ModelMetadata        (Option<f64> -> std::optional<double>)
//   error.rs:3-22       MagnetiteError{Input,Mesher,Solver,PostProcessor}, Display "<Kind> error: <msg>"
//   solver.rs:17-19     DOF, MAX_CG_ITER, TARGET_CG_COST
//   solver.rs:187-193   compute_element_area (pub; mesher.rs:9,523 imports it)
//   solver.rs:543-547   run(nodes, elements, model_metadata) -> Result<(), MagnetiteError>, mutating in place;
//                       afterwards every node.ux/uy/fx/fy and element.stress holds a value (solver.rs:476-482,532-533)
// The Rust shim a Magnetite maintainer would add instead is shown in INTEGRATION.md.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <optional>
#include <string>
#include <variant>
#include <vector>

#include "magnetite_hip.h"

namespace magnetite {

constexpr std::size_t DOF = MAG_DOF;                    // solver.rs:17
constexpr std::uint64_t MAX_CG_ITER = MAG_MAX_CG_ITER;  // solver.rs:18
constexpr double TARGET_CG_COST = MAG_TARGET_CG_COST;   // solver.rs:19

struct Vertex {  // datatypes.rs:1-5
    double x, y;
};
struct Node {  // datatypes.rs:7-14
    Vertex vertex;
    std::optional<double> ux, uy, fx, fy;
};
struct Element {  // datatypes.rs:16-20
    std::array<std::size_t, 3> nodes;
    std::optional<double> stress;
};
struct ModelMetadata {  // datatypes.rs:22-29
    double youngs_modulus, poisson_ratio, part_thickness;
    float characteristic_length_min = 0.f, characteristic_length_max = 0.f;
};

struct MagnetiteError {  // error.rs:3-22
    enum Kind { Input, Mesher, Solver, PostProcessor } kind;
    std::string message;
    std::string display() const
    {
        static const char *names[] = {"Input", "Mesher", "Solver", "Post Processor"};
        return std::string(names[kind]) + " error: " + message;
    }
};

// What solver::sensitivities returns per solved member: the outputs of mag_download_sensitivity, the scalars by name.
struct Sensitivity {
    std::vector<double> energy, dxy;
    double strain_energy = 0, potential_energy = 0, external_work = 0, reaction_work = 0, dPi_dE = 0, dPi_dnu = 0, dPi_dt = 0;
};

// What solver::adjoint returns per solved member: the outputs of mag_download_adjoint, the scalars by name.
struct Adjoint {
    std::vector<double> lambda, dloads, delem, dxy;
    double a = 0, dJ_dE = 0, dJ_dnu = 0, dJ_dt = 0;
};

// What solver::objective returns per solved member: the outputs of mag_download_objective, the scalars by name (pJ_*: explicit
// partials at fixed u; dxy and dJ_*: totals, filled when the adjoint ran).
struct Objective {
    std::vector<double> g, pxy, dxy;
    double J = 0, pJ_pE = 0, pJ_pnu = 0, pJ_pt = 0, dJ_dE = 0, dJ_dnu = 0, dJ_dt = 0;
    bool totals = false;
};

// What solver::stress_recovery returns per solved member: the outputs of mag_download_stress -- elem (E rows of sx, sy, txy, vm),
// node (N rows of the averaged tensor and its vm, in the order of `nodes`), eta2 (E) -- and the scalars by name: eta and
// energy_norm are the square roots of the library's eta^2 and U^2.
struct StressField {
    std::vector<double> elem, node, eta2;
    double eta = 0, energy_norm = 0, eta_rel = 0, vm_max = 0, vm_node_max = 0;
};

// What solver::modal returns: the outputs of mag_download_modal -- lambda ((rad/s)^2, ascending), frequency (Hz), residual, shapes
// (modes rows of 2N values in the order of `nodes`, mass-normalised, 0 on prescribed DOFs) -- and mag_get_modal_info's words by name.
struct Modes {
    std::vector<double> lambda, frequency, residual, shapes;
    std::int32_t modes = 0, subspace = 0, outer = 0, converged = 0, vectors_per_launch = 0, launches = 0, redone = 0;
};

// The options of solver::refine and solver::upload_refined (include/magnetite_hip.h, mag_refine_options).  marks (E values) given:
// MAG_REFINE_MARKS whatever `rule` says; otherwise `rule` of `indicator` (E values), or, when that is empty, of the ZZ indicator
// eta2 of the solved part, read on the device.
struct RefineSpec {
    std::int32_t rule = MAG_REFINE_TOP_FRACTION, split = 1;
    double theta = 0.2;
    std::vector<std::uint8_t> marks;
    std::vector<double> indicator;
};

// What solver::refine returns: the refined mesh as a part to solve -- nodes with their boundary data as posed (exactly one of
// displacement / force per axis), elements without stress --, the parents (node_parents: lo, hi of the edge that new node
// nodes.size() - node_parents.size() / 2 + i halves; elem_parent: the coarse element of every element) and mag_get_refine_info's
// words by name.
struct Refined {
    std::vector<Node> nodes;
    std::vector<Element> elements;
    std::vector<std::int32_t> node_parents, elem_parent;
    std::int64_t marked = 0, marked_edges = 0, sweeps = 0, split2 = 0, split3 = 0, split4 = 0;
};

// One solve of solver::upload_refined's loop: the mesh it ran on, the ZZ estimate of its solution, its CG iterations.
struct AdaptRound {
    std::size_t nodes = 0, elements = 0;
    double eta = 0, eta_rel = 0;
    std::int64_t iterations = 0;
};

// The options of solver::design_init (include/magnetite_hip.h, mag_design_options); rho0: E start densities in (0, 1], or empty:
// volume_fraction everywhere.
struct DesignSpec {
    double volume_fraction = 0.5, scale_min = 1e-3, rho_min = 1e-3, move = 0.2;
    std::int32_t penal = 3, filter_passes = 1;
    std::vector<double> rho0;
};

// mag_get_design_info's words by name.
struct DesignInfo {
    double volume_fraction = 0, lagrange = 0, change = 0, greyness = 0, J = 0;
    bool reachable = false;
    std::int64_t steps = 0;
};

// What solver::download_design returns: the outputs of mag_download_design, E values each.
struct Design {
    std::vector<double> rho, rho_filtered, scale, dJ_drho;
};

// A part kept on the device under an element stiffness field, between the calls of solver::set_element_scale, design_init,
// design_step, design_info and download_design.  Owns the context: it goes with this object on every path.
struct FieldSession {
    mag_ctx *ctx = nullptr;
    std::size_t N = 0, E = 0;
    FieldSession() = default;
    FieldSession(const FieldSession &) = delete;
    FieldSession &operator=(const FieldSession &) = delete;
    ~FieldSession()
    {
        if (ctx) mag_destroy(ctx);
    }
};

// The options of solver::modal (include/magnetite_hip.h, mag_modal_options); 0: the library's default.
struct ModalSpec {
    std::int32_t modes = 6, subspace = 0, max_outer = 0;
    bool lumped = false;
    double density = 0.0, tol = 0.0, cg_tol = 0.0;
};

// The options of solver::buckling (include/magnetite_hip.h, mag_buckling_options); 0: the library's default.
struct BucklingSpec {
    std::int32_t modes = 4, subspace = 0, max_outer = 0;
    double tol = 0.0, cg_tol = 0.0;
};

// What solver::buckling returns: the outputs of mag_download_buckling -- load_factor (signed, by magnitude ascending), residual,
// shapes (modes rows of 2N values in the order of `nodes`, K-normalised, 0 on prescribed DOFs) --, mag_get_buckling_info's words by
// name and critical: the smallest positive factor, if there is one.
struct BucklingModes {
    std::vector<double> load_factor, residual, shapes;
    std::int32_t modes = 0, subspace = 0, outer = 0, converged = 0, vectors_per_launch = 0, launches = 0, redone = 0, positive = 0;
    std::optional<double> critical;
};

// The options of solver::transient (include/magnetite_hip.h, mag_transient_options); 0: the library's default.  amplitude: steps + 1
// values or empty (ones); u0, v0: 2N values in the order of `nodes` or empty (zero); probes: DOF indices 2 * node + axis.
struct TransientSpec {
    std::int32_t steps = 0, cg = 0, snapshot_every = 0;
    bool lumped = false, energies = false;
    double dt = 0.0, beta = 0.25, gamma = 0.5, density = 0.0, rayleigh_mass = 0.0, rayleigh_stiffness = 0.0, cg_tol = 0.0;
    std::vector<double> amplitude, u0, v0;
    std::vector<std::int32_t> probes;
};

// What solver::transient returns: the outputs of mag_download_transient -- the final state u, v, a and its reactions f (2N each,
// in the order of `nodes`), the probes' rows (steps + 1 rows of probes.size() values), the energies (steps + 1 rows of T, W, P),
// the snapshots of u, the iterations per solve -- and mag_get_transient_info's words by name.
struct Transient {
    std::vector<double> u, v, a, f, probe_u, probe_v, probe_a, energies, snapshots;
    std::vector<std::int32_t> iterations;
    double t_start = 0, t_end = 0;
    std::int32_t steps = 0, cg_kernel = 0, preconditioner = 0, cg_iterations = 0, max_step_iterations = 0, snapshots_kept = 0, resumed = 0,
                 converged = 0;
};

// The options of solver::run_explicit (include/magnetite_hip.h, mag_explicit_options); dt 0: dt_scale times the device's bound.
// amplitude: steps + 1 values or empty (ones); u0, v0: 2N values in the order of `nodes` or empty (zero); probes: 2 * node + axis.
// kinematics: MAG_KIN_LINEAR, or MAG_KIN_TOTAL_LAGRANGIAN for large rotations (rayleigh_stiffness must then be 0).
struct ExplicitSpec {
    std::int32_t steps = 0, record_every = 1, snapshot_every = 0, kinematics = MAG_KIN_LINEAR;
    bool energies = false;
    double dt = 0.0, dt_scale = 0.9, density = 0.0, rayleigh_mass = 0.0, rayleigh_stiffness = 0.0;
    std::vector<double> amplitude, u0, v0;
    std::vector<std::int32_t> probes;
};

// What solver::run_explicit returns: the outputs of mag_download_transient after an explicit run -- the final state and its
// reactions, the rows of steps 0, record_every, ... (probes, energies, `time`), the snapshots -- the step used, its bound and
// mag_get_transient_info's words by name.  inverted: an element had det F <= 0 in a total-Lagrangian run (no error).
struct Explicit {
    std::vector<double> u, v, a, f, probe_u, probe_v, probe_a, energies, snapshots, time;
    double t_start = 0, t_end = 0, dt = 0, dt_bound = 0;
    std::int32_t steps = 0, method = 0, fused = 0, step_launches = 0, record_every = 0, snapshots_kept = 0, resumed = 0;
    bool inverted = false;
};

// What solver::internal_force returns (mag_internal_force): f_int(u) in the order of `nodes`, the strain energy W(u), and whether
// some element has det F <= 0.
struct InternalForce {
    std::vector<double> f;
    double energy = 0;
    bool inverted = false;
};

// The options of solver::run_newton (include/magnetite_hip.h, mag_newton_options).  load_factors: increments values or empty
// (k / increments); u0: 2N values in the order of `nodes` or empty (zero); probes: 2 * node + axis.
struct NewtonSpec {
    std::int32_t increments = 1, max_newton = 0, line_search = 0, cg = 0;
    bool snapshots = false;
    double newton_tol = 0.0, cg_tol = 0.0;
    std::vector<double> load_factors, u0;
    std::vector<std::int32_t> probes;
};

// What solver::run_newton returns: the outputs of mag_download_newton -- the last converged state, its reactions and element rows
// (E x 8: Exx, Eyy, Gxy, Sxx, Syy, Sxy, det F, W_e), the rows of the start and of every increment (load, probe_u, energies = W, Pi,
// newton_iterations, snapshots), one entry per Newton iteration of the run (residuals, cg_iterations, step_lengths) -- and
// mag_get_newton_info's words by name.  converged false: an increment ran into max_newton (no error); message says which.
struct Newton {
    std::vector<double> u, f, elem, probe_u, snapshots, load, energies, residuals, step_lengths;
    std::vector<std::int32_t> newton_iterations, cg_iterations;
    std::int32_t increments_converged = 0, cg_kernel = 0, preconditioner = 0, newton_iterations_total = 0, cg_iterations_total = 0, halvings = 0;
    bool inverted = false, converged = false;
    std::string message;
};

// The options of solver::transient_tl (include/magnetite_hip.h, mag_transient_tl_options); 0: the library's default.  amplitude,
// u0, v0 and probes as TransientSpec's.  There is no stiffness-proportional damping.
struct TransientTlSpec {
    std::int32_t steps = 0, cg = 0, snapshot_every = 0, max_newton = 0;
    bool lumped = false, energies = false;
    double dt = 0.0, beta = 0.25, gamma = 0.5, density = 0.0, rayleigh_mass = 0.0, cg_tol = 0.0, newton_tol = 0.0;
    std::vector<double> amplitude, u0, v0;
    std::vector<std::int32_t> probes;
};

// What solver::transient_tl returns: solver::transient's outputs (`run`: rows = steps done + 1; run.converged: every step
// converged) and the outputs of mag_download_transient_tl -- newton_iterations per step (entry 0 = 0), the residual ratio and the CG
// iterations of every Newton iteration of the run, the final state's element rows (E x 8, as Newton::elem) -- with
// mag_get_transient_tl_info's words by name.  converged false: a step ran into max_newton (no error); message says which.
struct TransientTl {
    Transient run;
    std::vector<std::int32_t> newton_iterations, newton_cg;
    std::vector<double> newton_residuals, elements;
    std::int32_t steps = 0, cg_kernel = 0, preconditioner = 0, newton_iterations_total = 0, max_step_newton = 0, cg_iterations_total = 0;
    bool inverted = false, converged = false;
    std::string message;
};

// What solver::explicit_dt returns (mag_explicit_dt)
struct ExplicitBound {
    double lambda_bound = 0, dt_bound_undamped = 0, dt_bound = 0, min_mass = 0;
};

// The objective of solver::objective (include/magnetite_hip.h, mag_objective): one row of weights (and of the target) for all
// members -- 2N values for MAG_OBJ_DISP_LSQ, E values or none for MAG_OBJ_STRESS_PNORM.
struct ObjectiveSpec {
    std::int32_t kind = MAG_OBJ_STRESS_PNORM;
    std::vector<double> weights, target;
    double p = 8.0, scale = 1.0;
};

// The objective of solver::adjoint: dJ/du (2N, already sized and zeroed, in the order of `nodes`) of member `member` at its
// solved displacements u (2N, prescribed values included).
using ObjectiveGradient = std::function<void(std::size_t member, const std::vector<double> &u, std::vector<double> &dJ_du)>;

// Result<(), MagnetiteError>
using Result = std::optional<MagnetiteError>;  // nullopt == Ok(())

namespace solver {

// solver.rs:187-193
inline double compute_element_area(const Element &element, const std::vector<Node> &nodes)
{
    const double xy[6] = {nodes[element.nodes[0]].vertex.x, nodes[element.nodes[0]].vertex.y,
                          nodes[element.nodes[1]].vertex.x, nodes[element.nodes[1]].vertex.y,
                          nodes[element.nodes[2]].vertex.x, nodes[element.nodes[2]].vertex.y};
    const std::int32_t tri[3] = {0, 1, 2};
    return mag_compute_element_area(xy, tri);
}

namespace detail {

inline Result solver_error(std::string m) { return Result(MagnetiteError{MagnetiteError::Solver, std::move(m)}); }

// Vec<Node> -> the C ABI's arrays (what the Rust shim does before the extern "C" call); with `mask_of`, the mask of another
// node list this one must agree with (load cases: one mask for all)
inline Result flatten_nodes(const std::vector<Node> &nodes, std::vector<double> &xy, std::vector<std::uint8_t> &u_known,
                            double *u_in, double *f_in, const std::vector<std::uint8_t> *mask_of = nullptr)
{
    const std::size_t N = nodes.size();
    xy.assign(2 * N, 0.0);
    u_known.assign(2 * N, 0);
    for (std::size_t i = 0; i < N; ++i) {
        xy[2 * i] = nodes[i].vertex.x;
        xy[2 * i + 1] = nodes[i].vertex.y;
        const std::optional<double> *uu[2] = {&nodes[i].ux, &nodes[i].uy}, *ff[2] = {&nodes[i].fx, &nodes[i].fy};
        for (int a = 0; a < 2; ++a) {
            u_in[2 * i + a] = f_in[2 * i + a] = 0.0;
            // exactly one of (u, f) per DOF; the reference panics otherwise (solver.rs:431,453,472)
            if (uu[a]->has_value() == ff[a]->has_value())
                return solver_error("node " + std::to_string(i) + ": exactly one of displacement/force must be prescribed per axis");
            if (uu[a]->has_value()) {
                u_known[2 * i + a] = 1;
                u_in[2 * i + a] = **uu[a];
            } else {
                f_in[2 * i + a] = **ff[a];
            }
            if (mask_of && (*mask_of)[2 * i + a] != u_known[2 * i + a])
                return solver_error("node " + std::to_string(i) + ": load cases must prescribe the same quantity per axis");
        }
    }
    return std::nullopt;
}

inline Result flatten_elements(const std::vector<Element> &elements, std::size_t N, std::vector<std::int32_t> &conn)
{
    const std::size_t E = elements.size();
    conn.assign(3 * E, 0);
    for (std::size_t e = 0; e < E; ++e)
        for (int c = 0; c < 3; ++c) {
            if (elements[e].nodes[c] >= N || elements[e].nodes[c] > 0x7fffffffu)
                return solver_error("element " + std::to_string(e) + " references a node outside the mesh");
            conn[3 * e + c] = (std::int32_t)elements[e].nodes[c];
        }
    return std::nullopt;
}

// the flattened arrays as the C ABI's problem (host memory)
inline mag_problem host_problem(const std::vector<double> &xy, const std::vector<std::int32_t> &conn,
                                const std::vector<std::uint8_t> &u_known, const double *u_in, const double *f_in,
                                const ModelMetadata &model_metadata)
{
    mag_problem p{};
    p.num_nodes = (std::int64_t)(xy.size() / 2);
    p.num_elements = (std::int64_t)(conn.size() / 3);
    p.xy = xy.data();
    p.conn = conn.data();
    p.u_known = u_known.data();
    p.u_in = u_in;
    p.f_in = f_in;
    p.youngs_modulus = model_metadata.youngs_modulus;
    p.poisson_ratio = model_metadata.poisson_ratio;
    p.part_thickness = model_metadata.part_thickness;
    p.memory = MAG_MEM_HOST;
    return p;
}

// the error path: the context's message, the context gone
inline Result fail_and_destroy(mag_ctx *ctx)
{
    Result e = solver_error(mag_last_error(ctx));
    mag_destroy(ctx);
    return e;
}

inline void store_values(std::vector<Node> &nodes, const std::vector<double> &u, const std::vector<double> &f)
{
    for (std::size_t i = 0; i < nodes.size(); ++i) {  // solver.rs:476-482
        nodes[i].ux = u[2 * i];
        nodes[i].uy = u[2 * i + 1];
        nodes[i].fx = f[2 * i];
        nodes[i].fy = f[2 * i + 1];
    }
}

// After a set's run (load cases, design variants) returned rc: the info words, every member's values into members[m], its
// stress and statistics; the context goes.  A member that broke down is an error, the others hold their results.
inline Result collect_members(mag_ctx *ctx, int rc, std::vector<std::vector<Node>> &members, std::size_t E,
                              std::vector<std::vector<double>> &stress, std::vector<mag_stats> *stats_out, std::int32_t *info_out,
                              int (*get_info)(const mag_ctx *, std::int32_t *), int (*download)(mag_ctx *, std::int32_t, mag_result *),
                              int (*get_stats)(const mag_ctx *, std::int32_t, mag_stats *))
{
    if (rc != MAG_OK && rc != MAG_ERR_NOT_CONVERGED) return fail_and_destroy(ctx);
    const std::string run_message = mag_last_error(ctx);
    const std::size_t M = members.size(), N = M ? members[0].size() : 0;
    std::vector<double> u(2 * N), f(2 * N);
    if (stats_out) stats_out->assign(M, mag_stats{});
    if (info_out) get_info(ctx, info_out);
    stress.assign(M, std::vector<double>(E));
    for (std::size_t m = 0; m < M; ++m) {
        mag_result r{};
        r.u_out = u.data();
        r.f_out = f.data();
        r.stress_out = stress[m].data();
        r.memory = MAG_MEM_HOST;
        if (download(ctx, (std::int32_t)m, &r) != MAG_OK) return fail_and_destroy(ctx);
        if (stats_out) get_stats(ctx, (std::int32_t)m, &(*stats_out)[m]);
        store_values(members[m], u, f);
    }
    mag_destroy(ctx);
    if (rc != MAG_OK) return solver_error(run_message);
    return std::nullopt;
}

// the variants' shapes and materials as mag_set_variants takes them: [V][2N] coordinates, [V][3] = E, nu, thickness
inline Result flatten_variants(const std::vector<std::vector<Vertex>> &shapes, const std::vector<ModelMetadata> &materials, std::size_t N,
                               std::vector<double> &vxy, std::vector<double> &vmat)
{
    for (std::size_t v = 0; v < shapes.size(); ++v) {
        if (shapes[v].size() != N) return solver_error("variant " + std::to_string(v) + " has another number of vertices");
        for (const Vertex &p : shapes[v]) {
            vxy.push_back(p.x);
            vxy.push_back(p.y);
        }
    }
    for (const ModelMetadata &m : materials) {
        vmat.push_back(m.youngs_modulus);
        vmat.push_back(m.poisson_ratio);
        vmat.push_back(m.part_thickness);
    }
    return std::nullopt;
}

// The solved members that sensitivities(), adjoint() and objective() differentiate: the part as it is -- shapes and materials
// both empty: one member, MAG_SET_RUN -- or its design variants as run_variants takes them (MAG_SET_VARIANTS).  Owns the context:
// it goes with this object on every path.
struct SolvedMembers {
    mag_ctx *ctx = nullptr;
    std::int32_t set = MAG_SET_RUN;
    std::size_t V = 0, N = 0, E = 0;
    SolvedMembers() = default;
    SolvedMembers(const SolvedMembers &) = delete;
    SolvedMembers &operator=(const SolvedMembers &) = delete;
    ~SolvedMembers()
    {
        if (ctx) mag_destroy(ctx);
    }
    // the error path: the context's message
    Result fail() const { return solver_error(mag_last_error(ctx)); }
    // The number of members before anything else is looked at, then `precheck` -- the caller's checks of its own arguments, which
    // sees V, N and E -- then flatten, create, upload, solve.
    template <class Precheck>
    Result solve(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                 const std::vector<std::vector<Vertex>> &shapes, const std::vector<ModelMetadata> &materials, const mag_options *options,
                 Precheck precheck)
    {
        const bool plain = shapes.empty() && materials.empty();
        set = plain ? MAG_SET_RUN : MAG_SET_VARIANTS;
        V = plain ? 1 : (shapes.empty() ? materials.size() : shapes.size()), N = nodes.size(), E = elements.size();
        if (!shapes.empty() && !materials.empty() && shapes.size() != materials.size())
            return solver_error("shapes and materials disagree on the number of variants");
        if (Result e = precheck()) return e;
        std::vector<double> xy, u_in(2 * N), f_in(2 * N), vxy, vmat;
        std::vector<std::uint8_t> u_known;
        std::vector<std::int32_t> conn;
        if (Result e = flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
        if (Result e = flatten_elements(elements, N, conn)) return e;
        if (Result e = flatten_variants(shapes, materials, N, vxy, vmat)) return e;
        ctx = mag_create(options);
        if (!ctx) return solver_error("mag_create failed");
        const mag_problem p = host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
        if (mag_upload(ctx, &p) != MAG_OK) return fail();
        if (set == MAG_SET_RUN) return mag_run(ctx) != MAG_OK ? fail() : std::nullopt;
        if (mag_set_variants(ctx, (std::int32_t)V, shapes.empty() ? nullptr : vxy.data(), materials.empty() ? nullptr : vmat.data(), nullptr,
                             nullptr, MAG_MEM_HOST) != MAG_OK)
            return fail();
        return mag_run_variants(ctx) != MAG_OK ? fail() : std::nullopt;
    }
};

}  // namespace detail

// solver.rs:543-586.  `options` == nullptr keeps the reference's constants (absolute cost 1e-4, 1e7 iterations).
inline Result run(std::vector<Node> &nodes, std::vector<Element> &elements, const ModelMetadata &model_metadata,
                  const mag_options *options = nullptr, mag_stats *stats_out = nullptr)
{
    auto err = detail::solver_error;
    const std::size_t N = nodes.size(), E = elements.size();
    std::vector<double> xy, u_in(2 * N, 0.0), f_in(2 * N, 0.0), u(2 * N), f(2 * N), stress(E);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return err("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    mag_result r{};
    r.u_out = u.data();
    r.f_out = f.data();
    r.stress_out = stress.data();
    r.memory = MAG_MEM_HOST;
    const int rc = mag_solve(ctx, &p, &r);
    if (stats_out) mag_get_stats(ctx, stats_out);
    if (rc != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_destroy(ctx);
    detail::store_values(nodes, u, f);
    for (std::size_t e = 0; e < E; ++e) elements[e].stress = stress[e];  // solver.rs:532-533
    return std::nullopt;
}

// Load cases (mag_set_load_cases / mag_run_cases): the same part under several sets of prescribed values.  cases[c] is the
// node list of case c -- the vertices of cases[0] and the same choice of prescribed quantity per axis, other values.  Order,
// symbolic work and K are done once, the CG solves run side by side on the chip where they fit; every case gets bit for bit
// what run() gives for it.  Afterwards every cases[c][i].ux/uy/fx/fy holds a value and stress[c][e] is element e's stress in
// case c (`elements` is shared by the cases and stays untouched).  info_out: mag_get_cases_info's four words.
inline Result run_cases(std::vector<std::vector<Node>> &cases, const std::vector<Element> &elements,
                        const ModelMetadata &model_metadata, std::vector<std::vector<double>> &stress,
                        const mag_options *options = nullptr, std::vector<mag_stats> *stats_out = nullptr,
                        std::int32_t *info_out = nullptr)
{
    auto err = detail::solver_error;
    if (cases.empty()) return err("no load case");
    const std::size_t L = cases.size(), N = cases[0].size(), E = elements.size();
    std::vector<double> xy, xy_c, u_in(L * 2 * N), f_in(L * 2 * N);
    std::vector<std::uint8_t> u_known, mask_c;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(cases[0], xy, u_known, u_in.data(), f_in.data())) return e;
    for (std::size_t c = 1; c < L; ++c) {
        if (cases[c].size() != N) return err("load case " + std::to_string(c) + " has another number of nodes");
        if (Result e = detail::flatten_nodes(cases[c], xy_c, mask_c, u_in.data() + c * 2 * N, f_in.data() + c * 2 * N, &u_known))
            return e;
        if (xy_c != xy) return err("load case " + std::to_string(c) + " has other vertices");
    }
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return err("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_set_load_cases(ctx, (std::int32_t)L, u_in.data(), f_in.data(), MAG_MEM_HOST) != MAG_OK) return detail::fail_and_destroy(ctx);
    return detail::collect_members(ctx, mag_run_cases(ctx), cases, E, stress, stats_out, info_out, mag_get_cases_info, mag_download_case,
                                   mag_get_case_stats);  // (a case broke down: the others hold their results)
}

// Design variants (mag_set_variants / mag_run_variants): the same part -- `nodes` and `elements`, which give the ordering every
// variant shares and stay untouched -- in several shapes and materials.  shapes: empty (every variant keeps the vertices of
// `nodes`) or one vertex list per variant; materials: empty (model_metadata for every variant) or one ModelMetadata per variant;
// at least one of the two is given, and both agree on the number of variants.  The prescribed values are those of `nodes`.
// Afterwards results[v][i].ux/uy/fx/fy hold variant v's values (vertex: the variant's) and stress[v][e] element e's stress.
// info_out: mag_get_variants_info's four words.
inline Result run_variants(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                           const std::vector<std::vector<Vertex>> &shapes, const std::vector<ModelMetadata> &materials,
                           std::vector<std::vector<Node>> &results, std::vector<std::vector<double>> &stress,
                           const mag_options *options = nullptr, std::vector<mag_stats> *stats_out = nullptr,
                           std::int32_t *info_out = nullptr)
{
    auto err = detail::solver_error;
    const std::size_t V = shapes.empty() ? materials.size() : shapes.size(), N = nodes.size(), E = elements.size();
    if (V == 0) return err("no variant: give shapes, materials or both");
    if (!shapes.empty() && !materials.empty() && shapes.size() != materials.size())
        return err("shapes and materials disagree on the number of variants");
    std::vector<double> xy, u_in(2 * N), f_in(2 * N), vxy, vmat;
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    if (Result e = detail::flatten_variants(shapes, materials, N, vxy, vmat)) return e;
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return err("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_set_variants(ctx, (std::int32_t)V, shapes.empty() ? nullptr : vxy.data(), materials.empty() ? nullptr : vmat.data(),
                         nullptr, nullptr, MAG_MEM_HOST) != MAG_OK)
        return detail::fail_and_destroy(ctx);
    const int rc = mag_run_variants(ctx);
    if (rc == MAG_OK || rc == MAG_ERR_NOT_CONVERGED) {
        results.assign(V, nodes);
        for (std::size_t v = 0; v < shapes.size(); ++v)
            for (std::size_t i = 0; i < N; ++i) results[v][i].vertex = shapes[v][i];
    }
    return detail::collect_members(ctx, rc, results, E, stress, stats_out, info_out, mag_get_variants_info, mag_download_variant,
                                   mag_get_variant_stats);  // (a variant broke down: the others hold their results)
}

// Energy and design sensitivities (mag_run_sensitivities) of the part as it is -- shapes and materials both empty: one member --
// or of its design variants, as run_variants takes them: the problem(s) are solved, then every member's element energies
// (energy, E values), the gradient of the potential energy with respect to every node coordinate (dxy, 2N values in the order of
// `nodes`; the problem is self-adjoint, no second solve) and the scalars of include/magnetite_hip.h by name.
inline Result sensitivities(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                            const std::vector<std::vector<Vertex>> &shapes, const std::vector<ModelMetadata> &materials,
                            std::vector<Sensitivity> &out, const mag_options *options = nullptr)
{
    detail::SolvedMembers sm;
    if (Result e = sm.solve(nodes, elements, model_metadata, shapes, materials, options, []() -> Result { return std::nullopt; })) return e;
    mag_ctx *ctx = sm.ctx;
    const std::int32_t set = sm.set;
    const std::size_t V = sm.V, N = sm.N, E = sm.E;
    if (mag_run_sensitivities(ctx, set) != MAG_OK) return sm.fail();
    out.assign(V, Sensitivity{});
    for (std::size_t v = 0; v < V; ++v) {
        Sensitivity &s = out[v];
        s.energy.resize(E);
        s.dxy.resize(2 * N);
        mag_sensitivity d{};
        d.energy_out = s.energy.data();
        d.dxy_out = s.dxy.data();
        d.memory = MAG_MEM_HOST;
        if (mag_download_sensitivity(ctx, set, (std::int32_t)v, &d) != MAG_OK) return sm.fail();
        s.strain_energy = d.scalars[0];
        s.potential_energy = d.scalars[1];
        s.external_work = d.scalars[2];
        s.reaction_work = d.scalars[3];
        s.dPi_dE = d.scalars[4];
        s.dPi_dnu = d.scalars[5];
        s.dPi_dt = d.scalars[6];
    }
    return std::nullopt;
}

// Adjoint sensitivities (mag_run_adjoint) of any objective J of the part as it is -- shapes and materials both empty: one member
// -- or of its design variants, as sensitivities() takes them: the problem(s) are solved, `objective` gives dJ/du at every
// member's u, one adjoint solve per member with the member's own K follows (side by side on the chip where the sets' solves
// are), then per member lambda, dJ/d(loads) (dloads), dJ/d(relative stiffness of an element) (delem), dJ/d(node coordinates)
// (dxy) and dJ/dE, dJ/dnu, dJ/dt -- total derivatives at fixed prescribed values; J's explicit dependence on the design is the
// caller's to add (include/magnetite_hip.h).  Under an absolute stop rule scale J so that |dJ/du| is of the size of the loads.
inline Result adjoint(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                      const std::vector<std::vector<Vertex>> &shapes, const std::vector<ModelMetadata> &materials,
                      const ObjectiveGradient &objective, std::vector<Adjoint> &out, const mag_options *options = nullptr)
{
    auto err = detail::solver_error;
    detail::SolvedMembers sm;
    const auto precheck = [&]() -> Result { return objective ? std::nullopt : err("no objective"); };
    if (Result e = sm.solve(nodes, elements, model_metadata, shapes, materials, options, precheck)) return e;
    mag_ctx *ctx = sm.ctx;
    const std::int32_t set = sm.set;
    const std::size_t V = sm.V, N = sm.N, E = sm.E;
    const bool plain = set == MAG_SET_RUN;
    std::vector<double> u(2 * N), g(V * 2 * N, 0.0), g_v;
    for (std::size_t v = 0; v < V; ++v) {
        mag_result r{};
        r.u_out = u.data();
        r.memory = MAG_MEM_HOST;
        if ((plain ? mag_download(ctx, &r) : mag_download_variant(ctx, (std::int32_t)v, &r)) != MAG_OK) return sm.fail();
        g_v.assign(2 * N, 0.0);
        objective(v, u, g_v);
        if (g_v.size() != 2 * N) return err("the objective resized dJ/du");
        std::copy(g_v.begin(), g_v.end(), g.begin() + v * 2 * N);
    }
    if (mag_run_adjoint(ctx, set, g.data(), MAG_MEM_HOST) != MAG_OK) return sm.fail();
    out.assign(V, Adjoint{});
    for (std::size_t v = 0; v < V; ++v) {
        Adjoint &s = out[v];
        s.lambda.resize(2 * N);
        s.dloads.resize(2 * N);
        s.delem.resize(E);
        s.dxy.resize(2 * N);
        mag_adjoint d{};
        d.lambda_out = s.lambda.data();
        d.dloads_out = s.dloads.data();
        d.delem_out = s.delem.data();
        d.dxy_out = s.dxy.data();
        d.memory = MAG_MEM_HOST;
        if (mag_download_adjoint(ctx, set, (std::int32_t)v, &d) != MAG_OK) return sm.fail();
        s.a = d.scalars[0];
        s.dJ_dE = d.scalars[1];
        s.dJ_dnu = d.scalars[2];
        s.dJ_dt = d.scalars[3];
    }
    return std::nullopt;
}

// An objective of the part as it is -- shapes and materials both empty: one member -- or of its design variants, as adjoint()
// takes them, evaluated on the device (mag_run_objective): the problem(s) are solved, then per member J, dJ/du (g) and J's explicit
// partials at fixed u (pxy, pJ_pE, pJ_pnu, pJ_pt); with_adjoint, dJ/du goes through the adjoint pass where it lies and the total
// derivatives dxy, dJ_dE, dJ_dnu, dJ_dt follow.  Under an absolute stop rule scale the weights so that |dJ/du| is of the size of
// the loads.
inline Result objective(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                        const std::vector<std::vector<Vertex>> &shapes, const std::vector<ModelMetadata> &materials,
                        const ObjectiveSpec &spec, bool with_adjoint, std::vector<Objective> &out, const mag_options *options = nullptr)
{
    auto err = detail::solver_error;
    detail::SolvedMembers sm;
    const auto precheck = [&]() -> Result {
        const std::size_t row = spec.kind == MAG_OBJ_DISP_LSQ ? 2 * sm.N : sm.E;
        if (!spec.weights.empty() && spec.weights.size() != row) return err("the objective's weights have another length than its sum");
        if (!spec.target.empty() && spec.target.size() != 2 * sm.N) return err("the objective's target has another length than 2 N");
        return std::nullopt;
    };
    if (Result e = sm.solve(nodes, elements, model_metadata, shapes, materials, options, precheck)) return e;
    mag_ctx *ctx = sm.ctx;
    const std::int32_t set = sm.set;
    const std::size_t V = sm.V, N = sm.N;
    mag_objective o{};
    o.kind = spec.kind;
    o.p = spec.p;
    o.scale = spec.scale;
    o.weights = spec.weights.empty() ? nullptr : spec.weights.data();
    o.target = spec.target.empty() ? nullptr : spec.target.data();
    o.memory = MAG_MEM_HOST;
    if (mag_run_objective(ctx, set, &o, with_adjoint ? 1 : 0) != MAG_OK) return sm.fail();
    out.assign(V, Objective{});
    for (std::size_t v = 0; v < V; ++v) {
        Objective &s = out[v];
        s.g.resize(2 * N);
        s.pxy.resize(2 * N);
        if (with_adjoint) s.dxy.resize(2 * N);
        mag_objective_result d{};
        d.g_out = s.g.data();
        d.pxy_out = s.pxy.data();
        d.dxy_out = with_adjoint ? s.dxy.data() : nullptr;
        d.memory = MAG_MEM_HOST;
        if (mag_download_objective(ctx, set, (std::int32_t)v, &d) != MAG_OK) return sm.fail();
        s.J = d.scalars[0];
        s.pJ_pE = d.scalars[1];
        s.pJ_pnu = d.scalars[2];
        s.pJ_pt = d.scalars[3];
        s.dJ_dE = d.scalars[4];
        s.dJ_dnu = d.scalars[5];
        s.dJ_dt = d.scalars[6];
        s.totals = d.scalars[7] != 0.0;
    }
    return std::nullopt;
}

// Stress recovery (mag_run_stress) of the part as it is -- shapes and materials both empty: one member -- or of its design
// variants, as sensitivities() takes them: the problem(s) are solved, then per member the stress tensor and von Mises value of
// every element, the area-weighted nodal field, the ZZ error indicator per element and the scalars of include/magnetite_hip.h by
// name.
inline Result stress_recovery(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                              const std::vector<std::vector<Vertex>> &shapes, const std::vector<ModelMetadata> &materials,
                              std::vector<StressField> &out, const mag_options *options = nullptr)
{
    detail::SolvedMembers sm;
    if (Result e = sm.solve(nodes, elements, model_metadata, shapes, materials, options, []() -> Result { return std::nullopt; })) return e;
    mag_ctx *ctx = sm.ctx;
    const std::int32_t set = sm.set;
    const std::size_t V = sm.V, N = sm.N, E = sm.E;
    if (mag_run_stress(ctx, set) != MAG_OK) return sm.fail();
    out.assign(V, StressField{});
    for (std::size_t v = 0; v < V; ++v) {
        StressField &s = out[v];
        s.elem.resize(4 * E);
        s.node.resize(4 * N);
        s.eta2.resize(E);
        mag_stress_field d{};
        d.elem_out = s.elem.data();
        d.node_out = s.node.data();
        d.eta2_out = s.eta2.data();
        d.memory = MAG_MEM_HOST;
        if (mag_download_stress(ctx, set, (std::int32_t)v, &d) != MAG_OK) return sm.fail();
        s.eta = std::sqrt(d.scalars[0]);
        s.energy_norm = std::sqrt(d.scalars[1]);
        s.eta_rel = d.scalars[2];
        s.vm_max = d.scalars[3];
        s.vm_node_max = d.scalars[4];
    }
    return std::nullopt;
}

// Modal analysis (mag_run_modal) of the part: the spec.modes lowest natural frequencies and mode shapes of K_FF phi = lambda M_FF phi
// with the density of spec (the model has none).  The DOFs of `nodes` with a displacement are supports whatever its value, the
// forces play no role; nothing is solved for them.  Reaching the cap of outer steps is no error: out.converged == 0.
inline Result modal(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                    const ModalSpec &spec, Modes &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_modal_options o{};
    o.modes = spec.modes;
    o.subspace = spec.subspace;
    o.max_outer = spec.max_outer;
    o.lumped = spec.lumped ? 1 : 0;
    o.density = spec.density;
    o.tol = spec.tol;
    o.cg_tol = spec.cg_tol;
    if (mag_run_modal(ctx, &o) != MAG_OK) return detail::fail_and_destroy(ctx);
    std::int32_t info[8] = {};
    if (mag_get_modal_info(ctx, info) != MAG_OK) return detail::fail_and_destroy(ctx);
    const std::size_t P = (std::size_t)info[0];
    out = Modes{};
    out.lambda.resize(P);
    out.frequency.resize(P);
    out.residual.resize(P);
    out.shapes.resize(P * 2 * N);
    mag_modal_result d{};
    d.lambda_out = out.lambda.data();
    d.frequency_out = out.frequency.data();
    d.residual_out = out.residual.data();
    d.shapes_out = out.shapes.data();
    d.memory = MAG_MEM_HOST;
    if (mag_download_modal(ctx, &d) != MAG_OK) return detail::fail_and_destroy(ctx);
    out.modes = info[0];
    out.subspace = info[1];
    out.outer = info[2];
    out.converged = info[3];
    out.vectors_per_launch = info[4];
    out.launches = info[5];
    out.redone = info[6];
    mag_destroy(ctx);
    return std::nullopt;
}

namespace detail {

// the part uploaded and solved once (mag_run): the prestress of the buckling entry points.  The context is the caller's on success
inline Result solved_part(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                          const mag_options *options, mag_ctx *&ctx)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = flatten_elements(elements, N, conn)) return e;
    ctx = mag_create(options);
    if (!ctx) return solver_error("mag_create failed");
    const mag_problem p = host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK || mag_run(ctx) != MAG_OK) return fail_and_destroy(ctx);
    return std::nullopt;
}

} // namespace detail

// Linearised buckling (mag_run_buckling) of the part under its own loads: the part is solved, then the spec.modes load factors of
// smallest magnitude of (K_FF + lambda K_G,FF) phi = 0 with their shapes.  The DOFs of `nodes` with a displacement are supports;
// lambda multiplies every force and every non-zero support displacement.  Reaching the cap of outer steps is no error:
// out.converged == 0.
inline Result buckling(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                       const BucklingSpec &spec, BucklingModes &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    mag_ctx *ctx = nullptr;
    if (Result e = detail::solved_part(nodes, elements, model_metadata, options, ctx)) return e;
    mag_buckling_options o{};
    o.modes = spec.modes;
    o.subspace = spec.subspace;
    o.max_outer = spec.max_outer;
    o.set = MAG_SET_RUN;
    o.tol = spec.tol;
    o.cg_tol = spec.cg_tol;
    if (mag_run_buckling(ctx, &o) != MAG_OK) return detail::fail_and_destroy(ctx);
    std::int32_t info[8] = {};
    if (mag_get_buckling_info(ctx, info) != MAG_OK) return detail::fail_and_destroy(ctx);
    const std::size_t P = (std::size_t)info[0];
    out = BucklingModes{};
    out.load_factor.resize(P);
    out.residual.resize(P);
    out.shapes.resize(P * 2 * N);
    mag_buckling_result d{};
    d.load_factor_out = out.load_factor.data();
    d.residual_out = out.residual.data();
    d.shapes_out = out.shapes.data();
    d.memory = MAG_MEM_HOST;
    if (mag_download_buckling(ctx, &d) != MAG_OK) return detail::fail_and_destroy(ctx);
    out.modes = info[0];
    out.subspace = info[1];
    out.outer = info[2];
    out.converged = info[3];
    out.vectors_per_launch = info[4];
    out.launches = info[5];
    out.redone = info[6];
    out.positive = info[7];
    for (double l : out.load_factor)
        if (l > 0.0 && (!out.critical || l < *out.critical)) out.critical = l;
    mag_destroy(ctx);
    return std::nullopt;
}

// y = K_G(sigma(u0)) x (2N values each, in the order of `nodes`) with the geometric stiffness of the solved part's stress
// (mag_apply_geometric); masked: prescribed DOFs zeroed on both sides.
inline Result apply_geometric(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                              const std::vector<double> &x, std::vector<double> &y, bool masked = false, const mag_options *options = nullptr)
{
    if (x.size() != 2 * nodes.size()) return detail::solver_error("x has another length than 2 N");
    mag_ctx *ctx = nullptr;
    if (Result e = detail::solved_part(nodes, elements, model_metadata, options, ctx)) return e;
    y.resize(x.size());
    if (mag_apply_geometric(ctx, MAG_SET_RUN, 0, x.data(), y.data(), masked ? 1 : 0) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_destroy(ctx);
    return std::nullopt;
}

// The geometric stiffness K_G(sigma(u0)) of the solved part's stress as a CSR matrix with mag_assemble_csr's pattern
// (mag_assemble_geometric).
inline Result assemble_geometric(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                                 std::vector<std::int32_t> &rowptr, std::vector<std::int32_t> &col, std::vector<double> &val,
                                 const mag_options *options = nullptr)
{
    mag_ctx *ctx = nullptr;
    if (Result e = detail::solved_part(nodes, elements, model_metadata, options, ctx)) return e;
    std::int64_t nnz = 0;
    if (mag_assemble_csr(ctx, &nnz, nullptr, nullptr, nullptr) != MAG_OK) return detail::fail_and_destroy(ctx);
    rowptr.resize(2 * nodes.size() + 1);
    col.resize((std::size_t)nnz);
    val.resize((std::size_t)nnz);
    if (mag_assemble_csr(ctx, &nnz, rowptr.data(), col.data(), nullptr) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_assemble_geometric(ctx, MAG_SET_RUN, 0, val.data(), MAG_MEM_HOST) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_destroy(ctx);
    return std::nullopt;
}

// Transient dynamics (mag_run_transient) of the part: spec.steps steps of Newmark's method with the density of spec (the model has
// none).  The DOFs of `nodes` with a displacement are supports held at that value for all time; the forces are the load, scaled
// by spec.amplitude step by step.  Nothing static is solved.  A solve that stops at the iteration cap is no error: out.converged == 0.
inline Result transient(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                        const TransientSpec &spec, Transient &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    if (!spec.amplitude.empty() && spec.amplitude.size() != (std::size_t)std::max(spec.steps, 0) + 1)
        return detail::solver_error("the amplitude has another length than steps + 1");
    if ((!spec.u0.empty() && spec.u0.size() != 2 * N) || (!spec.v0.empty() && spec.v0.size() != 2 * N))
        return detail::solver_error("u0 / v0 have another length than 2 N");
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_transient_options o;
    mag_default_transient_options(&o);
    o.steps = spec.steps;
    o.lumped = spec.lumped ? 1 : 0;
    o.cg = spec.cg;
    o.energies = spec.energies ? 1 : 0;
    o.snapshot_every = spec.snapshot_every;
    o.num_probes = (std::int32_t)spec.probes.size();
    o.memory = MAG_MEM_HOST;
    o.dt = spec.dt;
    o.beta = spec.beta;
    o.gamma = spec.gamma;
    o.density = spec.density;
    o.rayleigh_mass = spec.rayleigh_mass;
    o.rayleigh_stiffness = spec.rayleigh_stiffness;
    o.cg_tol = spec.cg_tol;
    o.amplitude = spec.amplitude.empty() ? nullptr : spec.amplitude.data();
    o.u0 = spec.u0.empty() ? nullptr : spec.u0.data();
    o.v0 = spec.v0.empty() ? nullptr : spec.v0.data();
    o.probes = spec.probes.empty() ? nullptr : spec.probes.data();
    if (mag_run_transient(ctx, &o) != MAG_OK) return detail::fail_and_destroy(ctx);
    std::int32_t info[8] = {};
    if (mag_get_transient_info(ctx, info) != MAG_OK) return detail::fail_and_destroy(ctx);
    const std::size_t rows = (std::size_t)info[0] + 1, P = spec.probes.size();
    out = Transient{};
    out.u.resize(2 * N);
    out.v.resize(2 * N);
    out.a.resize(2 * N);
    out.f.resize(2 * N);
    out.probe_u.resize(rows * P);
    out.probe_v.resize(rows * P);
    out.probe_a.resize(rows * P);
    if (spec.energies) out.energies.resize(3 * rows);
    out.snapshots.resize((std::size_t)info[5] * 2 * N);
    out.iterations.resize(rows);
    mag_transient_result d{};
    d.u_out = out.u.data();
    d.v_out = out.v.data();
    d.a_out = out.a.data();
    d.f_out = out.f.data();
    if (P) d.probe_u = out.probe_u.data(), d.probe_v = out.probe_v.data(), d.probe_a = out.probe_a.data();
    if (spec.energies) d.energies = out.energies.data();
    if (info[5]) d.snapshots = out.snapshots.data();
    d.iterations = out.iterations.data();
    d.memory = MAG_MEM_HOST;
    if (mag_download_transient(ctx, &d) != MAG_OK) return detail::fail_and_destroy(ctx);
    out.t_start = d.scalars[0];
    out.t_end = d.scalars[1];
    out.steps = info[0];
    out.cg_kernel = info[1];
    out.preconditioner = info[2];
    out.cg_iterations = info[3];
    out.max_step_iterations = info[4];
    out.snapshots_kept = info[5];
    out.resumed = info[6];
    out.converged = info[7];
    mag_destroy(ctx);
    return std::nullopt;
}

// The material law of the total-Lagrangian functions below (run_explicit with MAG_KIN_TOTAL_LAGRANGIAN, internal_force, run_newton,
// assemble_tangent, transient_tl, assemble_effective_tangent): every context they create is given it (mag_set_material_law).
// MAG_LAW_SVK by default; MAG_LAW_NEO_HOOKE: compressible neo-Hooke, plane stress enforced per element (include/magnetite_hip.h).
namespace detail {
inline std::int32_t &law_slot()
{
    static std::int32_t law = MAG_LAW_SVK;
    return law;
}
} // namespace detail
inline std::int32_t material_law() { return detail::law_slot(); }
inline Result set_material_law(std::int32_t law)
{
    if (law != MAG_LAW_SVK && law != MAG_LAW_NEO_HOOKE) return detail::solver_error("the material law is neither MAG_LAW_SVK nor MAG_LAW_NEO_HOOKE");
    detail::law_slot() = law;
    return std::nullopt;
}

// Explicit dynamics (mag_run_explicit) of the part: spec.steps central-difference steps on the lumped mass, one fused launch a
// step; supports, loads and the start as solver::transient.  (`explicit` is a keyword: hence the names.)
inline Result run_explicit(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                           const ExplicitSpec &spec, Explicit &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    if (!spec.amplitude.empty() && spec.amplitude.size() != (std::size_t)std::max(spec.steps, 0) + 1)
        return detail::solver_error("the amplitude has another length than steps + 1");
    if ((!spec.u0.empty() && spec.u0.size() != 2 * N) || (!spec.v0.empty() && spec.v0.size() != 2 * N))
        return detail::solver_error("u0 / v0 have another length than 2 N");
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_set_material_law(ctx, material_law()) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_explicit_options o;
    mag_default_explicit_options(&o);
    o.steps = spec.steps;
    o.energies = spec.energies ? 1 : 0;
    o.record_every = spec.record_every;
    o.snapshot_every = spec.snapshot_every;
    o.num_probes = (std::int32_t)spec.probes.size();
    o.memory = MAG_MEM_HOST;
    o.kinematics = spec.kinematics;
    o.dt = spec.dt;
    o.dt_scale = spec.dt_scale;
    o.density = spec.density;
    o.rayleigh_mass = spec.rayleigh_mass;
    o.rayleigh_stiffness = spec.rayleigh_stiffness;
    o.amplitude = spec.amplitude.empty() ? nullptr : spec.amplitude.data();
    o.u0 = spec.u0.empty() ? nullptr : spec.u0.data();
    o.v0 = spec.v0.empty() ? nullptr : spec.v0.data();
    o.probes = spec.probes.empty() ? nullptr : spec.probes.data();
    if (mag_run_explicit(ctx, &o) != MAG_OK) return detail::fail_and_destroy(ctx);
    std::int32_t info[8] = {};
    if (mag_get_transient_info(ctx, info) != MAG_OK) return detail::fail_and_destroy(ctx);
    const std::size_t rows = (std::size_t)(info[0] / info[4]) + 1, P = spec.probes.size();
    out = Explicit{};
    out.u.resize(2 * N);
    out.v.resize(2 * N);
    out.a.resize(2 * N);
    out.f.resize(2 * N);
    out.probe_u.resize(rows * P);
    out.probe_v.resize(rows * P);
    out.probe_a.resize(rows * P);
    if (spec.energies) out.energies.resize(3 * rows);
    out.snapshots.resize((std::size_t)info[5] * 2 * N);
    mag_transient_result d{};
    d.u_out = out.u.data();
    d.v_out = out.v.data();
    d.a_out = out.a.data();
    d.f_out = out.f.data();
    if (P) d.probe_u = out.probe_u.data(), d.probe_v = out.probe_v.data(), d.probe_a = out.probe_a.data();
    if (spec.energies) d.energies = out.energies.data();
    if (info[5]) d.snapshots = out.snapshots.data();
    d.memory = MAG_MEM_HOST;
    if (mag_download_transient(ctx, &d) != MAG_OK) return detail::fail_and_destroy(ctx);
    out.t_start = d.scalars[0];
    out.t_end = d.scalars[1];
    out.dt = d.scalars[2];
    out.dt_bound = d.scalars[3];
    out.steps = info[0];
    out.method = info[1];
    out.inverted = info[1] == 7 && info[7] == 0;
    out.fused = info[2];
    out.step_launches = info[3];
    out.record_every = info[4];
    out.snapshots_kept = info[5];
    out.resumed = info[6];
    out.time.resize(rows);
    for (std::size_t k = 0; k < rows; ++k) out.time[k] = out.t_start + out.dt * (double)((std::size_t)out.record_every * k);
    mag_destroy(ctx);
    return std::nullopt;
}

// The total-Lagrangian internal force of the part at the displacement u (2N values in the order of `nodes`): the residual of a
// caller's own dynamic relaxation or Newton loop (mag_internal_force).
inline Result internal_force(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                             const std::vector<double> &u, InternalForce &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    if (u.size() != 2 * N) return detail::solver_error("u has another length than 2 N");
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_set_material_law(ctx, material_law()) != MAG_OK) return detail::fail_and_destroy(ctx);
    out = InternalForce{};
    out.f.resize(2 * N);
    double scalars[2] = {};
    if (mag_internal_force(ctx, u.data(), out.f.data(), scalars, MAG_MEM_HOST) != MAG_OK) return detail::fail_and_destroy(ctx);
    out.energy = scalars[0];
    out.inverted = scalars[1] != 0.0;
    mag_destroy(ctx);
    return std::nullopt;
}

// Nonlinear statics (mag_run_newton) of the part: its large-deflection equilibrium under the total-Lagrangian internal force, in
// spec.increments load increments of Newton's method on the consistent tangent; supports and loads as solver::run.
inline Result run_newton(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                         const NewtonSpec &spec, Newton &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size(), E = elements.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    if (!spec.load_factors.empty() && spec.load_factors.size() != (std::size_t)std::max(spec.increments, 0))
        return detail::solver_error("the load factors have another length than increments");
    if (!spec.u0.empty() && spec.u0.size() != 2 * N) return detail::solver_error("u0 has another length than 2 N");
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_set_material_law(ctx, material_law()) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_newton_options o;
    mag_default_newton_options(&o);
    o.increments = spec.increments;
    o.max_newton = spec.max_newton;
    o.line_search = spec.line_search;
    o.cg = spec.cg;
    o.snapshots = spec.snapshots ? 1 : 0;
    o.num_probes = (std::int32_t)spec.probes.size();
    o.memory = MAG_MEM_HOST;
    o.newton_tol = spec.newton_tol;
    o.cg_tol = spec.cg_tol;
    o.load_factors = spec.load_factors.empty() ? nullptr : spec.load_factors.data();
    o.u0 = spec.u0.empty() ? nullptr : spec.u0.data();
    o.probes = spec.probes.empty() ? nullptr : spec.probes.data();
    if (mag_run_newton(ctx, &o) != MAG_OK) return detail::fail_and_destroy(ctx);
    std::int32_t info[8] = {};
    if (mag_get_newton_info(ctx, info) != MAG_OK) return detail::fail_and_destroy(ctx);
    const std::size_t rows = (std::size_t)spec.increments + 1, P = spec.probes.size(), its = (std::size_t)info[3];
    out = Newton{};
    out.u.resize(2 * N);
    out.f.resize(2 * N);
    out.elem.resize(8 * E);
    out.probe_u.resize(rows * P);
    if (spec.snapshots) out.snapshots.resize(rows * 2 * N);
    out.load.resize(rows);
    out.energies.resize(2 * rows);
    out.newton_iterations.resize(rows);
    out.residuals.resize(its);
    out.cg_iterations.resize(its);
    out.step_lengths.resize(its);
    mag_newton_result d{};
    d.u_out = out.u.data();
    d.f_out = out.f.data();
    d.elem = out.elem.data();
    if (P) d.probe_u = out.probe_u.data();
    if (spec.snapshots) d.snapshots = out.snapshots.data();
    d.load = out.load.data();
    d.energies = out.energies.data();
    d.newton_iterations = out.newton_iterations.data();
    if (its) d.residuals = out.residuals.data(), d.cg_iterations = out.cg_iterations.data(), d.step_lengths = out.step_lengths.data();
    d.memory = MAG_MEM_HOST;
    if (mag_download_newton(ctx, &d) != MAG_OK) return detail::fail_and_destroy(ctx);
    out.increments_converged = info[0];
    out.cg_kernel = info[1];
    out.preconditioner = info[2];
    out.newton_iterations_total = info[3];
    out.cg_iterations_total = info[4];
    out.halvings = info[5];
    out.inverted = info[6] != 0;
    out.converged = info[7] != 0;
    if (!out.converged) out.message = mag_last_error(ctx);
    mag_destroy(ctx);
    return std::nullopt;
}

// The consistent tangent K_T(u) of the total-Lagrangian internal force at the displacement u (2N values in the order of `nodes`)
// as a CSR matrix with mag_assemble_csr's pattern (mag_assemble_tangent).
inline Result assemble_tangent(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                               const std::vector<double> &u, std::vector<std::int32_t> &rowptr, std::vector<std::int32_t> &col,
                               std::vector<double> &val, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    if (u.size() != 2 * N) return detail::solver_error("u has another length than 2 N");
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_set_material_law(ctx, material_law()) != MAG_OK) return detail::fail_and_destroy(ctx);
    std::int64_t nnz = 0;
    if (mag_assemble_csr(ctx, &nnz, nullptr, nullptr, nullptr) != MAG_OK) return detail::fail_and_destroy(ctx);
    rowptr.resize(2 * N + 1);
    col.resize((std::size_t)nnz);
    val.resize((std::size_t)nnz);
    if (mag_assemble_csr(ctx, &nnz, rowptr.data(), col.data(), nullptr) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_assemble_tangent(ctx, u.data(), val.data(), MAG_MEM_HOST) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_destroy(ctx);
    return std::nullopt;
}

// Nonlinear transient dynamics (mag_run_transient_tl) of the part: spec.steps Newmark steps on the total-Lagrangian internal
// force, every step by Newton's method on the effective tangent; supports, loads and the start as solver::transient.  A step
// that does not converge within max_newton ends the run and is no error: out.converged is false, the state and the rows are the
// last converged step's.
inline Result transient_tl(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                           const TransientTlSpec &spec, TransientTl &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    if (!spec.amplitude.empty() && spec.amplitude.size() != (std::size_t)std::max(spec.steps, 0) + 1)
        return detail::solver_error("the amplitude has another length than steps + 1");
    if ((!spec.u0.empty() && spec.u0.size() != 2 * N) || (!spec.v0.empty() && spec.v0.size() != 2 * N))
        return detail::solver_error("u0 / v0 have another length than 2 N");
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_set_material_law(ctx, material_law()) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_transient_tl_options o;
    mag_default_transient_tl_options(&o);
    o.steps = spec.steps;
    o.lumped = spec.lumped ? 1 : 0;
    o.cg = spec.cg;
    o.energies = spec.energies ? 1 : 0;
    o.snapshot_every = spec.snapshot_every;
    o.num_probes = (std::int32_t)spec.probes.size();
    o.memory = MAG_MEM_HOST;
    o.max_newton = spec.max_newton;
    o.dt = spec.dt;
    o.beta = spec.beta;
    o.gamma = spec.gamma;
    o.density = spec.density;
    o.rayleigh_mass = spec.rayleigh_mass;
    o.cg_tol = spec.cg_tol;
    o.newton_tol = spec.newton_tol;
    o.amplitude = spec.amplitude.empty() ? nullptr : spec.amplitude.data();
    o.u0 = spec.u0.empty() ? nullptr : spec.u0.data();
    o.v0 = spec.v0.empty() ? nullptr : spec.v0.data();
    o.probes = spec.probes.empty() ? nullptr : spec.probes.data();
    if (mag_run_transient_tl(ctx, &o) != MAG_OK) return detail::fail_and_destroy(ctx);
    std::int32_t info[8] = {}, ti[8] = {};
    if (mag_get_transient_info(ctx, info) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_get_transient_tl_info(ctx, ti) != MAG_OK) return detail::fail_and_destroy(ctx);
    const std::size_t rows = (std::size_t)info[0] + 1, P = spec.probes.size(), its = (std::size_t)ti[3];
    out = TransientTl{};
    Transient &r = out.run;
    r.u.resize(2 * N);
    r.v.resize(2 * N);
    r.a.resize(2 * N);
    r.f.resize(2 * N);
    r.probe_u.resize(rows * P);
    r.probe_v.resize(rows * P);
    r.probe_a.resize(rows * P);
    if (spec.energies) r.energies.resize(3 * rows);
    r.snapshots.resize((std::size_t)info[5] * 2 * N);
    r.iterations.resize(rows);
    mag_transient_result d{};
    d.u_out = r.u.data();
    d.v_out = r.v.data();
    d.a_out = r.a.data();
    d.f_out = r.f.data();
    if (P) d.probe_u = r.probe_u.data(), d.probe_v = r.probe_v.data(), d.probe_a = r.probe_a.data();
    if (spec.energies) d.energies = r.energies.data();
    if (info[5]) d.snapshots = r.snapshots.data();
    d.iterations = r.iterations.data();
    d.memory = MAG_MEM_HOST;
    if (mag_download_transient(ctx, &d) != MAG_OK) return detail::fail_and_destroy(ctx);
    r.t_start = d.scalars[0];
    r.t_end = d.scalars[1];
    r.steps = info[0];
    r.cg_kernel = info[1];
    r.preconditioner = info[2];
    r.cg_iterations = info[3];
    r.max_step_iterations = info[4];
    r.snapshots_kept = info[5];
    r.resumed = info[6];
    r.converged = info[7];
    out.newton_iterations.resize(rows);
    out.newton_cg.resize(its);
    out.newton_residuals.resize(its);
    out.elements.resize(8 * elements.size());
    mag_transient_tl_result t{};
    t.newton_iterations = out.newton_iterations.data();
    if (its) t.cg_iterations = out.newton_cg.data(), t.residuals = out.newton_residuals.data();
    t.elem = out.elements.data();
    t.memory = MAG_MEM_HOST;
    if (mag_download_transient_tl(ctx, &t) != MAG_OK) return detail::fail_and_destroy(ctx);
    out.steps = ti[0];
    out.cg_kernel = ti[1];
    out.preconditioner = ti[2];
    out.newton_iterations_total = ti[3];
    out.max_step_newton = ti[4];
    out.cg_iterations_total = ti[5];
    out.inverted = ti[6] != 0;
    out.converged = ti[7] != 0;
    if (!out.converged) out.message = mag_last_error(ctx);
    mag_destroy(ctx);
    return std::nullopt;
}

// c_K K_T(u) + c_M M at the displacement u (2N values in the order of `nodes`) as a CSR matrix with mag_assemble_csr's pattern
// (mag_assemble_effective_tangent): the matrix of a Newton iteration of solver::transient_tl.
inline Result assemble_effective_tangent(const std::vector<Node> &nodes, const std::vector<Element> &elements,
                                         const ModelMetadata &model_metadata, const std::vector<double> &u, double c_K, double c_M,
                                         double density, bool lumped, std::vector<std::int32_t> &rowptr, std::vector<std::int32_t> &col,
                                         std::vector<double> &val, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    if (u.size() != 2 * N) return detail::solver_error("u has another length than 2 N");
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_set_material_law(ctx, material_law()) != MAG_OK) return detail::fail_and_destroy(ctx);
    std::int64_t nnz = 0;
    if (mag_assemble_csr(ctx, &nnz, nullptr, nullptr, nullptr) != MAG_OK) return detail::fail_and_destroy(ctx);
    rowptr.resize(2 * N + 1);
    col.resize((std::size_t)nnz);
    val.resize((std::size_t)nnz);
    if (mag_assemble_csr(ctx, &nnz, rowptr.data(), col.data(), nullptr) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (mag_assemble_effective_tangent(ctx, u.data(), c_K, c_M, density, lumped ? 1 : 0, val.data(), MAG_MEM_HOST) != MAG_OK)
        return detail::fail_and_destroy(ctx);
    mag_destroy(ctx);
    return std::nullopt;
}

// The bound of the stable explicit step of the part (mag_explicit_dt): Gershgorin on M_FF^-1 K_FF with the lumped mass.
inline Result explicit_dt(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                          double density, double rayleigh_stiffness, ExplicitBound &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    double b[4] = {};
    if (mag_explicit_dt(ctx, density, rayleigh_stiffness, b) != MAG_OK) return detail::fail_and_destroy(ctx);
    out = ExplicitBound{b[0], b[1], b[2], b[3]};
    mag_destroy(ctx);
    return std::nullopt;
}

namespace detail {

// mag_run_refine with spec on the uploaded (and, for the device's own indicator, solved and recovered) problem of ctx
inline int run_refine(mag_ctx *ctx, const RefineSpec &spec)
{
    mag_refine_options o{};
    o.rule = spec.marks.empty() ? spec.rule : (std::int32_t)MAG_REFINE_MARKS;
    o.split = spec.split;
    o.theta = spec.theta;
    o.marks = spec.marks.empty() ? nullptr : spec.marks.data();
    o.indicator = spec.indicator.empty() ? nullptr : spec.indicator.data();
    o.memory = MAG_MEM_HOST;
    return mag_run_refine(ctx, &o);
}

// mag_download_refine into a part as posed: the mask decides which of displacement / force a node's axis carries
inline int download_refined(mag_ctx *ctx, Refined &out)
{
    std::int64_t info[8] = {};
    if (int rc = mag_get_refine_info(ctx, info)) return rc;
    const std::size_t N = (std::size_t)info[0], E = (std::size_t)info[1], added = (std::size_t)info[3];
    std::vector<double> xy(2 * N), u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> known(2 * N);
    std::vector<std::int32_t> conn(3 * E);
    out = Refined{};
    out.node_parents.resize(2 * added);
    out.elem_parent.resize(E);
    mag_refined d{};
    d.xy = xy.data();
    d.conn = conn.data();
    d.u_known = known.data();
    d.u_in = u_in.data();
    d.f_in = f_in.data();
    d.node_parents = added ? out.node_parents.data() : nullptr;
    d.elem_parent = out.elem_parent.data();
    d.memory = MAG_MEM_HOST;
    if (int rc = mag_download_refine(ctx, &d)) return rc;
    out.nodes.resize(N);
    for (std::size_t i = 0; i < N; ++i) {
        Node &n = out.nodes[i];
        n.vertex = {xy[2 * i], xy[2 * i + 1]};
        if (known[2 * i]) n.ux = u_in[2 * i]; else n.fx = f_in[2 * i];
        if (known[2 * i + 1]) n.uy = u_in[2 * i + 1]; else n.fy = f_in[2 * i + 1];
    }
    out.elements.resize(E);
    for (std::size_t e = 0; e < E; ++e)
        out.elements[e].nodes = {(std::size_t)conn[3 * e], (std::size_t)conn[3 * e + 1], (std::size_t)conn[3 * e + 2]};
    out.marked = info[2];
    out.marked_edges = info[3];
    out.sweeps = info[4];
    out.split2 = info[5];
    out.split3 = info[6];
    out.split4 = info[7];
    return MAG_OK;
}

}  // namespace detail

// Mesh refinement (mag_run_refine): longest-edge bisection with conformity closure of the part's mesh, on the device.  With
// marks or an indicator in spec nothing is solved; otherwise the part is solved, its stress recovered, and the elements are
// marked by the ZZ indicator eta2 where it lies.  `nodes` carry the boundary data as posed; out.nodes carry the refined mesh's:
// old nodes keep theirs, a new node interpolates a constraint both of its parents carry and is free and unloaded otherwise.
inline Result refine(const std::vector<Node> &nodes, const std::vector<Element> &elements, const ModelMetadata &model_metadata,
                     const RefineSpec &spec, Refined &out, const mag_options *options = nullptr)
{
    const std::size_t N = nodes.size(), E = elements.size();
    if (!spec.marks.empty() && spec.marks.size() != E) return detail::solver_error("refine: marks must have one entry per element");
    if (!spec.indicator.empty() && spec.indicator.size() != E) return detail::solver_error("refine: indicator must have one entry per element");
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (spec.marks.empty() && spec.indicator.empty())
        if (mag_run(ctx) != MAG_OK || mag_run_stress(ctx, MAG_SET_RUN) != MAG_OK) return detail::fail_and_destroy(ctx);
    if (detail::run_refine(ctx, spec) != MAG_OK || detail::download_refined(ctx, out) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_destroy(ctx);
    return std::nullopt;
}

// The adaptive loop on mag_upload_refined, the mesh never leaving the device: per round solve -> mag_run_stress -> record ->
// mag_run_refine by the ZZ indicator (spec.rule, theta, split; marks and indicator are not used) -> mag_upload_refined; after
// the last refinement one more solve and recovery.  Afterwards `nodes` and
// `elements` are the final mesh as run() leaves a part -- every ux / uy / fx / fy and stress set --, history holds one entry
// per solve (rounds + 1) and *posed_out, when asked for, the final mesh's nodes with their boundary data
// as posed.
inline Result upload_refined(std::vector<Node> &nodes, std::vector<Element> &elements, const ModelMetadata &model_metadata,
                             const RefineSpec &spec, int rounds, std::vector<AdaptRound> &history, const mag_options *options = nullptr,
                             std::vector<Node> *posed_out = nullptr)
{
    std::size_t N = nodes.size(), E = elements.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = detail::flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = detail::flatten_elements(elements, N, conn)) return e;
    mag_ctx *ctx = mag_create(options);
    if (!ctx) return detail::solver_error("mag_create failed");
    const mag_problem p = detail::host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    if (mag_upload(ctx, &p) != MAG_OK) return detail::fail_and_destroy(ctx);
    RefineSpec by_eta2 = spec;
    by_eta2.marks.clear();
    by_eta2.indicator.clear();
    history.clear();
    bool refined = false;
    for (int r = 0;; ++r) {
        if (mag_run(ctx) != MAG_OK || mag_run_stress(ctx, MAG_SET_RUN) != MAG_OK) return detail::fail_and_destroy(ctx);
        mag_stress_field f{};
        f.memory = MAG_MEM_HOST;
        mag_stats st{};
        if (mag_download_stress(ctx, MAG_SET_RUN, 0, &f) != MAG_OK || mag_get_stats(ctx, &st) != MAG_OK) return detail::fail_and_destroy(ctx);
        history.push_back({N, E, std::sqrt(f.scalars[0]), f.scalars[2], st.iterations});
        if (r >= rounds) break;
        std::int64_t info[8] = {};
        if (detail::run_refine(ctx, by_eta2) != MAG_OK || mag_upload_refined(ctx) != MAG_OK || mag_get_refine_info(ctx, info) != MAG_OK)
            return detail::fail_and_destroy(ctx);
        N = (std::size_t)info[0];
        E = (std::size_t)info[1];
        refined = true;
    }
    Refined mesh;
    if (refined) {
        if (detail::download_refined(ctx, mesh) != MAG_OK) return detail::fail_and_destroy(ctx);
    } else {
        mesh.nodes = nodes;
        mesh.elements = elements;
    }
    std::vector<double> u(2 * N), f(2 * N), stress(E);
    mag_result res{};
    res.u_out = u.data();
    res.f_out = f.data();
    res.stress_out = stress.data();
    res.memory = MAG_MEM_HOST;
    if (mag_download(ctx, &res) != MAG_OK) return detail::fail_and_destroy(ctx);
    mag_destroy(ctx);
    if (posed_out) *posed_out = mesh.nodes;
    nodes = std::move(mesh.nodes);
    elements = std::move(mesh.elements);
    detail::store_values(nodes, u, f);
    for (std::size_t e = 0; e < E; ++e) elements[e].stress = stress[e];
    return std::nullopt;
}

namespace detail {

// the part of `nodes` and `elements` uploaded into a fresh context of the session
inline Result open_session(FieldSession &session, const std::vector<Node> &nodes, const std::vector<Element> &elements,
                           const ModelMetadata &model_metadata, const mag_options *options)
{
    const std::size_t N = nodes.size();
    std::vector<double> xy, u_in(2 * N), f_in(2 * N);
    std::vector<std::uint8_t> u_known;
    std::vector<std::int32_t> conn;
    if (Result e = flatten_nodes(nodes, xy, u_known, u_in.data(), f_in.data())) return e;
    if (Result e = flatten_elements(elements, N, conn)) return e;
    if (session.ctx) mag_destroy(session.ctx);
    session.ctx = mag_create(options);
    if (!session.ctx) return solver_error("mag_create failed");
    session.N = N;
    session.E = elements.size();
    const mag_problem p = host_problem(xy, conn, u_known, u_in.data(), f_in.data(), model_metadata);
    return mag_upload(session.ctx, &p) != MAG_OK ? solver_error(mag_last_error(session.ctx)) : std::nullopt;
}

}  // namespace detail

// NOTE on names: like the other functions of this namespace, the five below are whole workflows on a part, not the C entry points
// of the same name one to one -- and not what the Python methods of the same name do, which ARE the entry points alone:
// set_element_scale uploads, sets the field AND solves; design_init uploads and starts the design; design_step is one ITERATION
// (mag_run, mag_run_sensitivities, then mag_design_step).  A caller who wants the single calls has them on session.ctx.
//
// Element stiffness field (mag_set_element_scale): the part solved with K = sum_e scale[e] K_e.  The part is uploaded into the
// session, the field set (E values, finite and > 0) and the part solved (options->field_cg chooses the CG under the field:
// 0 the CSR operator's phase, 1 | 2 | 3 the fused block-row kernel, plain | Jacobi | block-Jacobi); afterwards every node.ux/uy/fx/fy and element.stress
// holds a value as after run() -- the stress is that of the unscaled material (include/magnetite_hip.h) -- and the session keeps
// the solved part for what follows (mag_run_sensitivities ... on session.ctx).
inline Result set_element_scale(FieldSession &session, std::vector<Node> &nodes, std::vector<Element> &elements,
                                const ModelMetadata &model_metadata, const std::vector<double> &scale, const mag_options *options = nullptr,
                                mag_stats *stats_out = nullptr)
{
    if (scale.size() != elements.size()) return detail::solver_error("element scale: one entry per element is needed");
    if (Result e = detail::open_session(session, nodes, elements, model_metadata, options)) return e;
    mag_ctx *ctx = session.ctx;
    const auto fail = [&]() { return detail::solver_error(mag_last_error(ctx)); };
    if (mag_set_element_scale(ctx, scale.data(), MAG_MEM_HOST) != MAG_OK || mag_run(ctx) != MAG_OK) return fail();
    std::vector<double> u(2 * session.N), f(2 * session.N), stress(session.E);
    mag_result r{};
    r.u_out = u.data();
    r.f_out = f.data();
    r.stress_out = stress.data();
    r.memory = MAG_MEM_HOST;
    if (mag_download(ctx, &r) != MAG_OK) return fail();
    if (stats_out) mag_get_stats(ctx, stats_out);
    detail::store_values(nodes, u, f);
    for (std::size_t e = 0; e < session.E; ++e) elements[e].stress = stress[e];
    return std::nullopt;
}

// Density design (mag_design_init): the part uploaded into the session and a design started on it -- the densities of spec, their
// filtered field and its SIMP scale, installed as the part's element scale.
inline Result design_init(FieldSession &session, const std::vector<Node> &nodes, const std::vector<Element> &elements,
                          const ModelMetadata &model_metadata, const DesignSpec &spec, const mag_options *options = nullptr)
{
    if (!spec.rho0.empty() && spec.rho0.size() != elements.size()) return detail::solver_error("design: rho0 needs one entry per element");
    if (Result e = detail::open_session(session, nodes, elements, model_metadata, options)) return e;
    mag_design_options o{};
    o.volume_fraction = spec.volume_fraction;
    o.scale_min = spec.scale_min;
    o.rho_min = spec.rho_min;
    o.move = spec.move;
    o.penal = spec.penal;
    o.filter_passes = spec.filter_passes;
    if (mag_design_init(session.ctx, &o, spec.rho0.empty() ? nullptr : spec.rho0.data(), MAG_MEM_HOST) != MAG_OK)
        return detail::solver_error(mag_last_error(session.ctx));
    return std::nullopt;
}

// mag_get_design_info by name
inline Result design_info(const FieldSession &session, DesignInfo &out)
{
    double info[8] = {};
    if (!session.ctx || mag_get_design_info(session.ctx, info) != MAG_OK) return detail::solver_error("design_info before design_init");
    out.volume_fraction = info[0];
    out.lagrange = info[1];
    out.change = info[2];
    out.greyness = info[3];
    out.reachable = info[4] != 0.0;
    out.steps = (std::int64_t)info[5];
    out.J = info[6];
    return std::nullopt;
}

// One iteration of the design loop (mag_run, mag_run_sensitivities, mag_design_step): the part is solved under the design's scale,
// then the densities take one optimality-criteria step under the volume constraint -- towards the stiffest design (J = -2 Pi) when
// dJ_ds is null, otherwise along the caller's dJ/ds_e (E values; the caller reads what it needs of the solved part from
// session.ctx in `objective`, which is called between the solve and the step).  info_out: the step's words; stats_out: the solve's.
inline Result design_step(FieldSession &session, DesignInfo *info_out = nullptr, mag_stats *stats_out = nullptr,
                          const std::function<Result(mag_ctx *, std::vector<double> &dJ_ds)> &objective = nullptr)
{
    mag_ctx *ctx = session.ctx;
    if (!ctx) return detail::solver_error("design_step before design_init");
    const auto fail = [&]() { return detail::solver_error(mag_last_error(ctx)); };
    if (mag_run(ctx) != MAG_OK) return fail();
    if (stats_out) mag_get_stats(ctx, stats_out);
    if (objective) {
        std::vector<double> dJ_ds(session.E, 0.0);
        if (Result e = objective(ctx, dJ_ds)) return e;
        if (mag_design_step(ctx, dJ_ds.data(), MAG_MEM_HOST) != MAG_OK) return fail();
    } else if (mag_run_sensitivities(ctx, MAG_SET_RUN) != MAG_OK || mag_design_step(ctx, nullptr, MAG_MEM_HOST) != MAG_OK) {
        return fail();
    }
    return info_out ? design_info(session, *info_out) : std::nullopt;
}

// mag_download_design: the design as it stands
inline Result download_design(FieldSession &session, Design &out)
{
    if (!session.ctx) return detail::solver_error("download_design before design_init");
    out.rho.assign(session.E, 0.0);
    out.rho_filtered.assign(session.E, 0.0);
    out.scale.assign(session.E, 0.0);
    out.dJ_drho.assign(session.E, 0.0);
    mag_design d{};
    d.rho_out = out.rho.data();
    d.rho_filtered_out = out.rho_filtered.data();
    d.scale_out = out.scale.data();
    d.dJ_drho_out = out.dJ_drho.data();
    d.memory = MAG_MEM_HOST;
    return mag_download_design(session.ctx, &d) != MAG_OK ? detail::solver_error(mag_last_error(session.ctx)) : std::nullopt;
}

}  // namespace solver
}  // namespace magnetite
