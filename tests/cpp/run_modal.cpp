// Compiled-caller check of solver::modal (include/magnetite_solver.hpp) on the problem in the file it is given (written by
// tests/test_modal_cpp.py from the tensile fixture: "N E youngs nu t", then per node "x y known_x known_y ux uy fx fy", then per
// element its three nodes; floats hexadecimal).  Prints every result as a hexadecimal double, for the test to compare bit for bit
// with the Python binding's.
#include <cstdio>

#include "magnetite_solver.hpp"

using namespace magnetite;

int main(int argc, char **argv)
{
    std::FILE *in = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
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
    ModalSpec spec;
    spec.modes = 4;
    spec.density = 2700.0;
    Modes m;
    if (Result e = solver::modal(nodes, elements, meta, spec, m)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = m.modes == 4 && m.lambda.size() == 4 && m.frequency.size() == 4 && m.residual.size() == 4 && m.shapes.size() == 4 * 2 * N;
    std::printf("info %d %d %d %d %d %d %d\n", m.modes, m.subspace, m.outer, m.converged, m.vectors_per_launch, m.launches, m.redone);
    for (std::size_t k = 0; ok && k < 4; ++k) {
        double sum = 0.0;
        for (std::size_t d = 0; d < 2 * N; ++d) sum += m.shapes[k * 2 * N + d];
        std::printf("mode %zu %a %a %a sum %a\n", k, m.lambda[k], m.frequency[k], m.residual[k], sum);
    }
    // options the library refuses are an error, not a crash
    spec.density = 0.0;
    Result e2 = solver::modal(nodes, elements, meta, spec, m);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
