// Compiled-caller check of solver::transient_tl and solver::assemble_effective_tangent (include/magnetite_solver.hpp) on the problem
// in the file it is given (written by tests/test_transient_tl_cpp.py from plate16 under a pull of 5 %: "N E youngs nu t", then per
// node "x y known_x known_y ux uy fx fy", then per element its three nodes; floats hexadecimal): 6 steps of dt = argv[2] from
// u0_x = 0.05 (x - x_min) under the mass damping argv[3] (both hexadecimal), energies, snapshots every 2, three probes.  Prints
// every result as a hexadecimal double, for the test to compare bit for bit with the Python binding's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "magnetite_solver.hpp"

using namespace magnetite;

int main(int argc, char **argv)
{
    std::FILE *in = argc > 3 ? std::fopen(argv[1], "r") : nullptr;
    if (!in) {
        std::printf("FAIL no problem file\n");
        return 2;
    }
    std::size_t N = 0, E = 0;
    ModelMetadata meta{};
    bool ok = std::fscanf(in, "%zu %zu %la %la %la", &N, &E, &meta.youngs_modulus, &meta.poisson_ratio, &meta.part_thickness) == 5;
    std::vector<Node> nodes;
    std::vector<double> xs;
    for (std::size_t i = 0; ok && i < N; ++i) {
        double x, y, ux, uy, fx, fy;
        int kx, ky;
        ok = std::fscanf(in, "%la %la %d %d %la %la %la %la", &x, &y, &kx, &ky, &ux, &uy, &fx, &fy) == 8;
        Node n{{x, y}, std::nullopt, std::nullopt, std::nullopt, std::nullopt};
        if (kx) n.ux = ux; else n.fx = fx;
        if (ky) n.uy = uy; else n.fy = fy;
        nodes.push_back(n);
        xs.push_back(x);
    }
    std::vector<Element> elements;
    for (std::size_t e = 0; ok && e < E; ++e) {
        std::size_t a, b, c;
        ok = std::fscanf(in, "%zu %zu %zu", &a, &b, &c) == 3;
        elements.push_back({{a, b, c}, std::nullopt});
    }
    std::fclose(in);
    if (!ok || N == 0) {
        std::printf("FAIL the problem file does not parse\n");
        return 2;
    }
    const double x_min = *std::min_element(xs.begin(), xs.end());
    TransientTlSpec spec;
    spec.steps = 6;
    spec.dt = std::strtod(argv[2], nullptr);
    spec.density = 2700.0;
    spec.rayleigh_mass = std::strtod(argv[3], nullptr);
    spec.energies = true;
    spec.snapshot_every = 2;
    spec.newton_tol = 1e-10;
    spec.cg_tol = 1e-12;
    spec.probes = {3, (std::int32_t)N, (std::int32_t)(2 * N - 1)};
    spec.u0.assign(2 * N, 0.0);
    for (std::size_t i = 0; i < N; ++i) spec.u0[2 * i] = 0.05 * (xs[i] - x_min);
    TransientTl tt;
    if (Result e = solver::transient_tl(nodes, elements, meta, spec, tt)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    const Transient &r = tt.run;
    ok = tt.steps == 6 && tt.converged && !tt.inverted && r.steps == 6 && r.u.size() == 2 * N && r.f.size() == 2 * N && r.probe_u.size() == 7 * 3 &&
         r.energies.size() == 7 * 3 && r.snapshots.size() == 4 * 2 * N && r.iterations.size() == 7 && tt.newton_iterations.size() == 7 &&
         tt.newton_residuals.size() == (std::size_t)tt.newton_iterations_total && tt.elements.size() == 8 * E;
    std::printf("info %d %d %d %d %d %d %d %d\n", tt.steps, tt.cg_kernel, tt.preconditioner, tt.newton_iterations_total, tt.max_step_newton,
                tt.cg_iterations_total, tt.inverted ? 1 : 0, tt.converged ? 1 : 0);
    std::printf("run %d %d %d %d %d %d %d %d\n", r.steps, r.cg_kernel, r.preconditioner, r.cg_iterations, r.max_step_iterations, r.snapshots_kept,
                r.resumed, r.converged);
    std::printf("time %a %a\n", r.t_start, r.t_end);
    std::vector<std::int32_t> rowptr, col;
    std::vector<double> val;
    if (Result e = solver::assemble_effective_tangent(nodes, elements, meta, r.u, 0.25 * spec.dt * spec.dt, 1.0, spec.density, false, rowptr, col, val)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ok && rowptr.size() == 2 * N + 1 && val.size() == (std::size_t)rowptr.back() && col.size() == val.size();
    const std::vector<double> *vectors[] = {&r.u, &r.v, &r.a, &r.f, &r.snapshots, &r.energies, &tt.newton_residuals, &tt.elements, &val};
    const char *names[] = {"u", "v", "a", "f", "snapshots", "energies", "newton_residuals", "elements", "effective_tangent"};
    for (int k = 0; ok && k < 9; ++k) {
        double sum = 0.0;
        for (double x : *vectors[k]) sum += x;
        std::printf("sum %s %a\n", names[k], sum);
    }
    std::size_t at = 0;
    for (std::size_t n = 0; ok && n < 7; ++n) {
        int cg = 0;
        for (int i = 0; i < tt.newton_iterations[n]; ++i) cg += tt.newton_cg[at + (std::size_t)i];
        at += (std::size_t)tt.newton_iterations[n];
        ok = ok && (n == 0 || cg == r.iterations[n]); // (a step's CG iterations are its Newton iterations' summed)
        std::printf("step %zu %d %d", n, (int)tt.newton_iterations[n], (int)r.iterations[n]);
        for (std::size_t k = 0; k < 3; ++k) std::printf(" %a %a %a", r.probe_u[3 * n + k], r.probe_v[3 * n + k], r.probe_a[3 * n + k]);
        std::printf("\n");
    }
    // what the library refuses is an error, not a crash: beta = 0, a short u; a cap that is too low is none
    spec.beta = 0.0;
    Result e2 = solver::transient_tl(nodes, elements, meta, spec, tt);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0 && e2->display().find("mag_run_explicit") != std::string::npos;
    spec.beta = 0.25;
    Result e3 = solver::assemble_effective_tangent(nodes, elements, meta, std::vector<double>(3), 1.0, 1.0, spec.density, false, rowptr, col, val);
    ok = ok && e3.has_value() && e3->display().rfind("Solver error:", 0) == 0;
    spec.max_newton = 1;
    Result e4 = solver::transient_tl(nodes, elements, meta, spec, tt);
    ok = ok && !e4.has_value() && !tt.converged && tt.steps == 0 && tt.run.iterations.size() == 1 && tt.message.find("step 1") != std::string::npos;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
