// Compiled-caller check of solver::stress_recovery (include/magnetite_solver.hpp) on the problem in the file it is given (written
// by tests/test_stress_recovery_cpp.py from the tensile fixture: "N E youngs nu t", then per node "x y known_x known_y ux uy fx fy",
// then per element its three nodes; floats hexadecimal), solved once as it is and once in three materials.  Prints every result
// as a hexadecimal double, for the test to compare bit for bit with the Python binding's.
#include <cstdio>

#include "magnetite_solver.hpp"

using namespace magnetite;

static void print(const char *what, int i, const StressField &s)
{
    double se = 0.0, sn = 0.0, sz = 0.0;
    for (double v : s.elem) se += v;
    for (double v : s.node) sn += v;
    for (double v : s.eta2) sz += v;
    std::printf("%s %d sums %a %a %a scalars %a %a %a %a %a\n", what, i, se, sn, sz, s.eta, s.energy_norm, s.eta_rel, s.vm_max, s.vm_node_max);
}

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
    const std::vector<ModelMetadata> materials = {{69e9, 0.33, 0.5}, {110e9, 0.25, 0.75}, {40e9, 0.38, 0.3}};
    std::vector<StressField> one, three;
    if (Result e = solver::stress_recovery(nodes, elements, meta, {}, {}, one)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    if (Result e = solver::stress_recovery(nodes, elements, meta, {}, materials, three)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = one.size() == 1 && three.size() == 3;
    for (std::size_t i = 0; i < one.size(); ++i) print("run", (int)i, one[i]);
    for (std::size_t i = 0; i < three.size(); ++i) print("variant", (int)i, three[i]);
    for (const StressField &s : three) ok = ok && s.elem.size() == 4 * E && s.node.size() == 4 * N && s.eta2.size() == E;
    // a material mag_upload would refuse is an error, not a crash
    Result e2 = solver::stress_recovery(nodes, elements, meta, {}, {{69e9, 1.0, 0.5}}, three);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
