// Compiled-caller check of solver::run_variants (include/magnetite_solver.hpp): the patch-test mesh of run_patch.cpp in three
// materials.  Prints every result as a hexadecimal double, for tests/test_variants_cpp.py to compare bit for bit with the
// Python binding's.
#include <cstdio>

#include "magnetite_solver.hpp"

using namespace magnetite;

int main()
{
    const int nx = 12, ny = 6;
    const double L = 2.0, H = 1.0;
    std::vector<Node> nodes;
    for (int j = 0; j <= ny; ++j)
        for (int i = 0; i <= nx; ++i) {
            Node n{{L * i / nx, H * j / ny}, std::nullopt, std::nullopt, 0.0, 0.0};
            if (i == 0) { n.ux = 0.0; n.fx = std::nullopt; if (j == 0) { n.uy = 0.0; n.fy = std::nullopt; } }
            if (i == nx) { n.ux = 1e-3; n.fx = std::nullopt; }
            nodes.push_back(n);
        }
    std::vector<Element> elements;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const std::size_t a = j * (nx + 1) + i, b = a + 1, c = a + nx + 1, d = c + 1;
            elements.push_back({{a, b, d}, std::nullopt});
            elements.push_back({{a, d, c}, std::nullopt});
        }
    const ModelMetadata meta{69e9, 0.33, 0.5};
    const std::vector<ModelMetadata> materials = {{69e9, 0.33, 0.5}, {110e9, 0.25, 0.75}, {40e9, 0.38, 0.3}};
    std::vector<std::vector<Node>> results;
    std::vector<std::vector<double>> stress;
    std::vector<mag_stats> st;
    std::int32_t info[4] = {0, 0, 0, 0};
    if (Result e = solver::run_variants(nodes, elements, meta, {}, materials, results, stress, nullptr, &st, info)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    std::printf("info %d %d %d %d\n", (int)info[0], (int)info[1], (int)info[2], (int)info[3]);
    for (int v = 0; v < 3; ++v) {
        double su = 0.0, sf = 0.0, ss = 0.0;
        for (const Node &n : results[v]) {
            su += *n.ux + *n.uy;
            sf += *n.fx + *n.fy;
        }
        for (double s : stress[v]) ss += s;
        std::printf("variant %d iterations %lld sums %a %a %a\n", v, (long long)st[v].iterations, su, sf, ss);
    }
    // a material mag_upload would refuse, and no variant at all, are errors, not crashes
    Result e2 = solver::run_variants(nodes, elements, meta, {}, {{69e9, 1.0, 0.5}}, results, stress);
    Result e3 = solver::run_variants(nodes, elements, meta, {}, {}, results, stress);
    const bool ok = e2.has_value() && e2->display().rfind("Solver error:", 0) == 0 && e3.has_value();
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
