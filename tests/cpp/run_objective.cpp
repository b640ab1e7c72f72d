// Compiled-caller check of solver::objective (include/magnetite_solver.hpp) on a problem read from a text file (argv[1]; the test
// writes the tensile fixture into it): "N E youngs nu thickness", then per node "x y known_x known_y ux uy fx fy", per element its
// three nodes, then "p scale", E weights of the stress p-norm, 2N weights and 2N targets of the least squares.  Both objectives,
// with the adjoint, once on the problem as it is and once in three materials.  Prints every result as a hexadecimal double, for
// tests/test_objective_cpp.py to compare bit for bit with the Python binding's.
#include <cstdio>

#include "magnetite_solver.hpp"

using namespace magnetite;

static void print(const char *kind, const char *what, int i, const Objective &s)
{
    double sums[3] = {0.0, 0.0, 0.0};
    for (double v : s.g) sums[0] += v * v;
    for (double v : s.pxy) sums[1] += v * v;
    for (double v : s.dxy) sums[2] += v * v;
    std::printf("%s %s %d sums %a %a %a scalars %a %a %a %a %a %a %a\n", kind, what, i, sums[0], sums[1], sums[2], s.J, s.pJ_pE, s.pJ_pnu,
                s.pJ_pt, s.dJ_dE, s.dJ_dnu, s.dJ_dt);
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
    ObjectiveSpec pnorm, lsq;
    pnorm.kind = MAG_OBJ_STRESS_PNORM;
    lsq.kind = MAG_OBJ_DISP_LSQ;
    ok = ok && std::fscanf(in, "%la %la", &pnorm.p, &pnorm.scale) == 2;
    pnorm.weights.resize(E);
    lsq.weights.resize(2 * N);
    lsq.target.resize(2 * N);
    for (std::size_t i = 0; ok && i < E; ++i) ok = std::fscanf(in, "%la", &pnorm.weights[i]) == 1;
    for (std::size_t i = 0; ok && i < 2 * N; ++i) ok = std::fscanf(in, "%la", &lsq.weights[i]) == 1;
    for (std::size_t i = 0; ok && i < 2 * N; ++i) ok = std::fscanf(in, "%la", &lsq.target[i]) == 1;
    std::fclose(in);
    if (!ok) {
        std::printf("FAIL malformed input file\n");
        return 2;
    }
    const std::vector<ModelMetadata> materials = {meta, {110e9, 0.25, 0.75}, {40e9, 0.38, 0.3}};
    const ObjectiveSpec *specs[2] = {&pnorm, &lsq};
    const char *names[2] = {"stress_pnorm", "disp_lsq"};
    for (int k = 0; k < 2; ++k) {
        std::vector<Objective> one, three;
        if (Result e = solver::objective(nodes, elements, meta, {}, {}, *specs[k], true, one)) {
            std::printf("FAIL %s\n", e->display().c_str());
            return 2;
        }
        if (Result e = solver::objective(nodes, elements, meta, {}, materials, *specs[k], true, three)) {
            std::printf("FAIL %s\n", e->display().c_str());
            return 2;
        }
        ok = ok && one.size() == 1 && three.size() == 3;
        for (std::size_t i = 0; i < one.size(); ++i) print(names[k], "run", (int)i, one[i]);
        for (std::size_t i = 0; i < three.size(); ++i) print(names[k], "variant", (int)i, three[i]);
        for (const Objective &s : three) ok = ok && s.totals && s.g.size() == 2 * N && s.pxy.size() == 2 * N && s.dxy.size() == 2 * N;
    }
    // without the adjoint there are no totals; an argument the library refuses is an error, not a crash
    std::vector<Objective> plain;
    Result e1 = solver::objective(nodes, elements, meta, {}, {}, pnorm, false, plain);
    ok = ok && !e1.has_value() && plain.size() == 1 && !plain[0].totals && plain[0].dxy.empty() && plain[0].dJ_dE == 0.0;
    ObjectiveSpec bad = pnorm;
    bad.p = 0.5;
    Result e2 = solver::objective(nodes, elements, meta, {}, {}, bad, false, plain);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    bad = lsq;
    bad.weights.clear();
    Result e3 = solver::objective(nodes, elements, meta, {}, {}, bad, false, plain);
    ok = ok && e3.has_value();
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
