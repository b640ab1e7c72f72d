// Compiled-caller check of solver::run_explicit with kinematics = MAG_KIN_TOTAL_LAGRANGIAN and of solver::internal_force
// (include/magnetite_solver.hpp) on the problem in the file it is given (written by tests/test_explicit_tl_cpp.py from plate16 under
// a pull of 5 %: "N E youngs nu t", then per node "x y known_x known_y ux uy fx fy", then per element its three nodes; floats
// hexadecimal): 40 steps at the device's own step from u0_x = 0.05 (x - x_min), rows every 4, snapshots every 8, the mass damping in
// argv[2] (hexadecimal).  Prints every result as a hexadecimal double, for the test to compare bit for bit with the Python binding's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "magnetite_solver.hpp"

using namespace magnetite;

int main(int argc, char **argv)
{
    std::FILE *in = argc > 2 ? std::fopen(argv[1], "r") : nullptr;
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
    ExplicitSpec spec;
    spec.steps = 40;
    spec.density = 2700.0;
    spec.rayleigh_mass = std::strtod(argv[2], nullptr);
    spec.energies = true;
    spec.record_every = 4;
    spec.snapshot_every = 8;
    spec.kinematics = MAG_KIN_TOTAL_LAGRANGIAN;
    spec.probes = {3, (std::int32_t)N, (std::int32_t)(2 * N - 1)};
    spec.u0.assign(2 * N, 0.0);
    for (std::size_t i = 0; i < N; ++i) spec.u0[2 * i] = 0.05 * (xs[i] - x_min);
    Explicit ex;
    if (Result e = solver::run_explicit(nodes, elements, meta, spec, ex)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ex.steps == 40 && ex.method == 7 && !ex.inverted && ex.u.size() == 2 * N && ex.f.size() == 2 * N && ex.probe_u.size() == 11 * 3 &&
         ex.energies.size() == 11 * 3 && ex.snapshots.size() == 6 * 2 * N && ex.time.size() == 11;
    std::printf("info %d %d %d %d %d %d %d\n", ex.steps, ex.method, ex.fused, ex.step_launches, ex.record_every, ex.snapshots_kept, ex.resumed);
    std::printf("time %a %a %a %a\n", ex.t_start, ex.t_end, ex.dt, ex.dt_bound);
    InternalForce fi;
    if (Result e = solver::internal_force(nodes, elements, meta, spec.u0, fi)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ok && fi.f.size() == 2 * N && !fi.inverted;
    std::printf("energy %a\n", fi.energy);
    const std::vector<double> *vectors[] = {&ex.u, &ex.v, &ex.a, &ex.f, &ex.snapshots, &ex.energies, &ex.time, &fi.f};
    const char *names[] = {"u", "v", "a", "f", "snapshots", "energies", "time", "f_int"};
    for (int k = 0; ok && k < 8; ++k) {
        double sum = 0.0;
        for (double x : *vectors[k]) sum += x;
        std::printf("sum %s %a\n", names[k], sum);
    }
    for (std::size_t n = 0; ok && n < 11; ++n) {
        std::printf("row %zu", n);
        for (std::size_t k = 0; k < 3; ++k) std::printf(" %a %a %a", ex.probe_u[3 * n + k], ex.probe_v[3 * n + k], ex.probe_a[3 * n + k]);
        std::printf("\n");
    }
    // options the library refuses are an error, not a crash: stiffness-proportional damping, an unknown kinematics, a short u
    spec.rayleigh_stiffness = 1e-7;
    Result e2 = solver::run_explicit(nodes, elements, meta, spec, ex);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0 && e2->display().find("rayleigh_stiffness") != std::string::npos;
    spec.rayleigh_stiffness = 0.0;
    spec.kinematics = 2;
    Result e3 = solver::run_explicit(nodes, elements, meta, spec, ex);
    ok = ok && e3.has_value() && e3->display().find("kinematics") != std::string::npos;
    Result e4 = solver::internal_force(nodes, elements, meta, std::vector<double>(3), fi);
    ok = ok && e4.has_value() && e4->display().rfind("Solver error:", 0) == 0;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
