// Compiled-caller check of solver::adjoint (include/magnetite_solver.hpp) on a problem read from a text file (argv[1]; the test
// writes the tensile fixture into it): "N E youngs nu thickness", then per node "x y known_x known_y ux uy fx fy", per element its
// three nodes, then 2N weights w of the objective J = sum w u^2.  Solved once as it is and once in three materials.  Prints
// every result as a hexadecimal double, for tests/test_adjoint_cpp.py to compare bit for bit with the Python binding's.
#include <cstdio>

#include "magnetite_solver.hpp"

using namespace magnetite;

static void print(const char *what, int i, const Adjoint &s)
{
    double sums[4] = {0.0, 0.0, 0.0, 0.0};
    for (double v : s.lambda) sums[0] += v * v;
    for (double v : s.dloads) sums[1] += v * v;
    for (double v : s.delem) sums[2] += v;
    for (double v : s.dxy) sums[3] += v * v;
    std::printf("%s %d sums %a %a %a %a scalars %a %a %a %a\n", what, i, sums[0], sums[1], sums[2], sums[3], s.a, s.dJ_dE, s.dJ_dnu, s.dJ_dt);
}

int main(int argc, char **argv)
{
    std::FILE *in = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
    if (!in) {
        std::printf("FAIL no input file\n");
        return 2;
    }
    std::size_t N = 0, E = 0;
    ModelMetadata meta{};
    bool ok = std::fscanf(in, "%zu %zu %la %la %la", &N, &E, &meta.youngs_modulus, &meta.poisson_ratio, &meta.part_thickness) == 5;
    std::vector<Node> nodes;
    for (std::size_t i = 0; ok && i < N; ++i) {
        double x, y, u[2], f[2];
        int k[2];
        ok = std::fscanf(in, "%la %la %d %d %la %la %la %la", &x, &y, &k[0], &k[1], &u[0], &u[1], &f[0], &f[1]) == 8;
        Node n{{x, y}, std::nullopt, std::nullopt, std::nullopt, std::nullopt};
        if (k[0]) n.ux = u[0]; else n.fx = f[0];
        if (k[1]) n.uy = u[1]; else n.fy = f[1];
        nodes.push_back(n);
    }
    std::vector<Element> elements;
    for (std::size_t e = 0; ok && e < E; ++e) {
        std::size_t a, b, c;
        ok = std::fscanf(in, "%zu %zu %zu", &a, &b, &c) == 3;
        elements.push_back({{a, b, c}, std::nullopt});
    }
    std::vector<double> w(2 * N);
    for (std::size_t i = 0; ok && i < 2 * N; ++i) ok = std::fscanf(in, "%la", &w[i]) == 1;
    std::fclose(in);
    if (!ok) {
        std::printf("FAIL malformed input file\n");
        return 2;
    }
    const ObjectiveGradient objective = [&](std::size_t, const std::vector<double> &u, std::vector<double> &g) {
        for (std::size_t i = 0; i < u.size(); ++i) g[i] = 2.0 * w[i] * u[i];
    };
    const std::vector<ModelMetadata> materials = {meta, {110e9, 0.25, 0.75}, {40e9, 0.38, 0.3}};
    std::vector<Adjoint> one, three;
    if (Result e = solver::adjoint(nodes, elements, meta, {}, {}, objective, one)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    if (Result e = solver::adjoint(nodes, elements, meta, {}, materials, objective, three)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = one.size() == 1 && three.size() == 3;
    for (std::size_t i = 0; i < one.size(); ++i) print("run", (int)i, one[i]);
    for (std::size_t i = 0; i < three.size(); ++i) print("variant", (int)i, three[i]);
    for (const Adjoint &s : three)
        ok = ok && s.lambda.size() == 2 * N && s.dloads.size() == 2 * N && s.delem.size() == E && s.dxy.size() == 2 * N;
    // a material mag_upload would refuse is an error, not a crash; so is a missing objective
    Result e2 = solver::adjoint(nodes, elements, meta, {}, {{69e9, 1.0, 0.5}}, objective, three);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    Result e3 = solver::adjoint(nodes, elements, meta, {}, {}, ObjectiveGradient(), three);
    ok = ok && e3.has_value();
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
