// Compiled-caller check of solver::transient (include/magnetite_solver.hpp) on the problem in the file it is given (written by
// tests/test_transient_cpp.py from the tensile fixture: "N E youngs nu t", then per node "x y known_x known_y ux uy fx fy", then
// per element its three nodes; floats hexadecimal), 16 steps of the dt in argv[2] (hexadecimal).  Prints every result as a
// hexadecimal double, for the test to compare bit for bit with the Python binding's.
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
    TransientSpec spec;
    spec.steps = 16;
    spec.dt = std::strtod(argv[2], nullptr);
    spec.density = 2700.0;
    spec.energies = true;
    spec.snapshot_every = 8;
    spec.probes = {3, (std::int32_t)N, (std::int32_t)(2 * N - 1)};
    Transient tr;
    if (Result e = solver::transient(nodes, elements, meta, spec, tr)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = tr.steps == 16 && tr.u.size() == 2 * N && tr.f.size() == 2 * N && tr.probe_u.size() == 17 * 3 && tr.energies.size() == 17 * 3 &&
         tr.snapshots.size() == 3 * 2 * N && tr.iterations.size() == 17;
    std::printf("info %d %d %d %d %d %d %d %d\n", tr.steps, tr.cg_kernel, tr.preconditioner, tr.cg_iterations, tr.max_step_iterations,
                tr.snapshots_kept, tr.resumed, tr.converged);
    std::printf("time %a %a\n", tr.t_start, tr.t_end);
    const std::vector<double> *vectors[] = {&tr.u, &tr.v, &tr.a, &tr.f, &tr.snapshots, &tr.energies};
    const char *names[] = {"u", "v", "a", "f", "snapshots", "energies"};
    for (int k = 0; ok && k < 6; ++k) {
        double sum = 0.0;
        for (double x : *vectors[k]) sum += x;
        std::printf("sum %s %a\n", names[k], sum);
    }
    for (std::size_t n = 0; ok && n < 17; ++n) {
        std::printf("step %zu %d", n, (int)tr.iterations[n]);
        for (std::size_t k = 0; k < 3; ++k) std::printf(" %a %a %a", tr.probe_u[3 * n + k], tr.probe_v[3 * n + k], tr.probe_a[3 * n + k]);
        std::printf("\n");
    }
    // options the library refuses are an error, not a crash
    spec.density = 0.0;
    Result e2 = solver::transient(nodes, elements, meta, spec, tr);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
