// Compiled-caller check of solver::run_cases (include/magnetite_solver.hpp): the patch-test mesh of run_patch.cpp under two
// load sets.  Prints every result as a hexadecimal double, for tests/test_load_cases_cpp.py to compare bit for bit with the
// Python binding's.
#include <cstdio>

#include "magnetite_solver.hpp"

using namespace magnetite;

int main()
{
    const int nx = 12, ny = 6;
    const double L = 2.0, H = 1.0;
    const double delta[2] = {1e-3, 2.5e-4}, pull[2] = {0.0, 1.0e4};
    std::vector<std::vector<Node>> cases(2);
    for (int c = 0; c < 2; ++c)
        for (int j = 0; j <= ny; ++j)
            for (int i = 0; i <= nx; ++i) {
                Node n{{L * i / nx, H * j / ny}, std::nullopt, std::nullopt, 0.0, 0.0};
                if (i == 0) { n.ux = 0.0; n.fx = std::nullopt; if (j == 0) { n.uy = 0.0; n.fy = std::nullopt; } }
                if (i == nx) { n.ux = delta[c]; n.fx = std::nullopt; }
                if (j == ny && i > 0 && i < nx) n.fy = pull[c]; // case 1 also pulls the top edge
                cases[c].push_back(n);
            }
    std::vector<Element> elements;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const std::size_t a = j * (nx + 1) + i, b = a + 1, c = a + nx + 1, d = c + 1;
            elements.push_back({{a, b, d}, std::nullopt});
            elements.push_back({{a, d, c}, std::nullopt});
        }
    const ModelMetadata meta{69e9, 0.33, 0.5};
    std::vector<std::vector<double>> stress;
    std::vector<mag_stats> st;
    std::int32_t info[4] = {0, 0, 0, 0};
    if (Result e = solver::run_cases(cases, elements, meta, stress, nullptr, &st, info)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    std::printf("info %d %d %d %d\n", (int)info[0], (int)info[1], (int)info[2], (int)info[3]);
    for (int c = 0; c < 2; ++c) {
        std::printf("case %d iterations %lld\n", c, (long long)st[c].iterations);
        for (const Node &n : cases[c]) std::printf("n %a %a %a %a\n", *n.ux, *n.uy, *n.fx, *n.fy);
        for (double s : stress[c]) std::printf("s %a\n", s);
    }
    // another mask in a later case is an error, not a crash
    cases[1][5].fx = std::nullopt;
    cases[1][5].ux = 0.0;
    Result e2 = solver::run_cases(cases, elements, meta, stress);
    const bool ok = e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
