// Compiled-caller check of solver::sensitivities (include/magnetite_solver.hpp): the patch-test mesh of run_patch.cpp, solved
// once as it is and once in three materials.  Prints every result as a hexadecimal double, for tests/test_sensitivities_cpp.py
// to compare bit for bit with the Python binding's.
#include <cstdio>

#include "magnetite_solver.hpp"

using namespace magnetite;

static void print(const char *what, int i, const Sensitivity &s)
{
    double se = 0.0, sg = 0.0;
    for (double v : s.energy) se += v;
    for (double v : s.dxy) sg += v * v;
    std::printf("%s %d sums %a %a scalars %a %a %a %a %a %a %a\n", what, i, se, sg, s.strain_energy, s.potential_energy, s.external_work,
                s.reaction_work, s.dPi_dE, s.dPi_dnu, s.dPi_dt);
}

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
            if (j == ny && i > 0 && i < nx) n.fy = 1.0e4;
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
    std::vector<Sensitivity> one, three;
    if (Result e = solver::sensitivities(nodes, elements, meta, {}, {}, one)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    if (Result e = solver::sensitivities(nodes, elements, meta, {}, materials, three)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    bool ok = one.size() == 1 && three.size() == 3;
    for (std::size_t i = 0; i < one.size(); ++i) print("run", (int)i, one[i]);
    for (std::size_t i = 0; i < three.size(); ++i) print("variant", (int)i, three[i]);
    for (const Sensitivity &s : three) ok = ok && s.energy.size() == elements.size() && s.dxy.size() == 2 * nodes.size();
    // a material mag_upload would refuse is an error, not a crash
    Result e2 = solver::sensitivities(nodes, elements, meta, {}, {{69e9, 1.0, 0.5}}, three);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
