// Compiled-caller check of solver::run_explicit and solver::explicit_dt (include/magnetite_solver.hpp) on the problem in the file
// it is given (written by tests/test_explicit_cpp.py from plate16: "N E youngs nu t", then per node "x y known_x known_y ux uy fx
// fy", then per element its three nodes; floats hexadecimal): 40 steps at the device's own step, rows every 4, snapshots every 8,
// the damping in argv[2], argv[3] (hexadecimal).  Prints every result as a hexadecimal double, for the test to compare bit for
// bit with the Python binding's.
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
    for (std::size_t i = 0; ok && i < N; ++i) {
        double x, y, ux, uy, fx, fy;
        int kx, ky;
        ok = std::fscanf(in, "%la %la %d %d %la %la %la %la", &x, &y, &kx, &ky, &ux, &uy, &fx, &fy) == 8;
        Node n{{x, y}, std::nullopt, std::nullopt, std::nullopt, std::nullopt};
        if (kx) n.ux = ux; else n.fx = fx;
        if (ky) n.uy = uy; else n.fy = fy;
        nodes.push_back(n);
    }
    std::vector<Element> elements;
    for (std::size_t e = 0; ok && e < E; ++e) {
        std::size_t a, b, c;
        ok = std::fscanf(in, "%zu %zu %zu", &a, &b, &c) == 3;
        elements.push_back({{a, b, c}, std::nullopt});
    }
    std::fclose(in);
    if (!ok) {
        std::printf("FAIL the problem file does not parse\n");
        return 2;
    }
    ExplicitSpec spec;
    spec.steps = 40;
    spec.density = 2700.0;
    spec.rayleigh_mass = std::strtod(argv[2], nullptr);
    spec.rayleigh_stiffness = std::strtod(argv[3], nullptr);
    spec.energies = true;
    spec.record_every = 4;
    spec.snapshot_every = 8;
    spec.probes = {3, (std::int32_t)N, (std::int32_t)(2 * N - 1)};
    ExplicitBound bound;
    if (Result e = solver::explicit_dt(nodes, elements, meta, spec.density, spec.rayleigh_stiffness, bound)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    std::printf("bound %a %a %a %a\n", bound.lambda_bound, bound.dt_bound_undamped, bound.dt_bound, bound.min_mass);
    Explicit ex;
    if (Result e = solver::run_explicit(nodes, elements, meta, spec, ex)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ex.steps == 40 && ex.u.size() == 2 * N && ex.f.size() == 2 * N && ex.probe_u.size() == 11 * 3 && ex.energies.size() == 11 * 3 &&
         ex.snapshots.size() == 6 * 2 * N && ex.time.size() == 11 && ex.dt_bound == bound.dt_bound;
    std::printf("info %d %d %d %d %d %d\n", ex.steps, ex.fused, ex.step_launches, ex.record_every, ex.snapshots_kept, ex.resumed);
    std::printf("time %a %a %a %a\n", ex.t_start, ex.t_end, ex.dt, ex.dt_bound);
    const std::vector<double> *vectors[] = {&ex.u, &ex.v, &ex.a, &ex.f, &ex.snapshots, &ex.energies, &ex.time};
    const char *names[] = {"u", "v", "a", "f", "snapshots", "energies", "time"};
    for (int k = 0; ok && k < 7; ++k) {
        double sum = 0.0;
        for (double x : *vectors[k]) sum += x;
        std::printf("sum %s %a\n", names[k], sum);
    }
    for (std::size_t n = 0; ok && n < 11; ++n) {
        std::printf("row %zu", n);
        for (std::size_t k = 0; k < 3; ++k) std::printf(" %a %a %a", ex.probe_u[3 * n + k], ex.probe_v[3 * n + k], ex.probe_a[3 * n + k]);
        std::printf("\n");
    }
    // options the library refuses are an error, not a crash
    spec.density = 0.0;
    Result e2 = solver::run_explicit(nodes, elements, meta, spec, ex);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    Result e3 = solver::explicit_dt(nodes, elements, meta, -1.0, 0.0, bound);
    ok = ok && e3.has_value() && e3->display().rfind("Solver error:", 0) == 0;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
