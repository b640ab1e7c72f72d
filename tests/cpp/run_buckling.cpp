// Compiled-caller check of solver::buckling, solver::apply_geometric and solver::assemble_geometric (include/magnetite_solver.hpp) on
// the problem in the file it is given (written by tests/test_buckling_cpp.py from the column8 part of tests/buckling_ref.py, in
// run_modal.cpp's format: "N E youngs nu t", then per node "x y known_x known_y ux uy fx fy", then per element its three nodes;
// floats hexadecimal).  Prints every result as a hexadecimal double, for the test to compare bit for bit with the Python binding's.
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
    BucklingSpec spec;
    spec.modes = 6;
    spec.subspace = 14;
    spec.max_outer = 60;
    BucklingModes m;
    if (Result e = solver::buckling(nodes, elements, meta, spec, m)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = m.modes == 6 && m.load_factor.size() == 6 && m.residual.size() == 6 && m.shapes.size() == 6 * 2 * N && m.critical.has_value();
    std::printf("info %d %d %d %d %d %d %d %d\n", m.modes, m.subspace, m.outer, m.converged, m.vectors_per_launch, m.launches, m.redone, m.positive);
    if (ok) std::printf("critical %a\n", *m.critical);
    for (std::size_t k = 0; ok && k < 6; ++k) {
        double sum = 0.0;
        for (std::size_t d = 0; d < 2 * N; ++d) sum += m.shapes[k * 2 * N + d];
        std::printf("mode %zu %a %a sum %a\n", k, m.load_factor[k], m.residual[k], sum);
    }
    // the operator and the assembled matrix on the same vector: x_d = 1 / (1 + d)
    std::vector<double> x(2 * N), y, val;
    std::vector<std::int32_t> rowptr, col;
    for (std::size_t d = 0; d < 2 * N; ++d) x[d] = 1.0 / (1.0 + (double)d);
    if (Result e = solver::apply_geometric(nodes, elements, meta, x, y)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    if (Result e = solver::assemble_geometric(nodes, elements, meta, rowptr, col, val)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ok && y.size() == 2 * N && rowptr.size() == 2 * N + 1 && (std::size_t)rowptr[2 * N] == val.size() && col.size() == val.size();
    double ysum = 0.0, vsum = 0.0, worst = 0.0, scale = 0.0;
    for (std::size_t r = 0; ok && r < 2 * N; ++r) {
        double s = 0.0;
        for (std::int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) s += val[(std::size_t)k] * x[(std::size_t)col[(std::size_t)k]];
        worst = std::fmax(worst, std::fabs(s - y[r]));
        scale = std::fmax(scale, std::fabs(y[r]));
        ysum += y[r];
    }
    for (double v : val) vsum += v;
    std::printf("operator %a values %a\n", ysum, vsum);
    ok = ok && scale > 0.0 && worst <= 1e-12 * scale; // (the assembled matrix applies as the operator does)
    // options the library refuses are an error, not a crash
    spec.modes = 0;
    Result e2 = solver::buckling(nodes, elements, meta, spec, m);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
