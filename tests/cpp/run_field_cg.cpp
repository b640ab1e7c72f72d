// Compiled-caller check of mag_options.field_cg through include/magnetite_solver.hpp: the problem in the file it is given (written
// by tests/test_field_cg_cpp.py from plate(6, 5), in run_design.cpp's format) solved under an element stiffness field with
// field_cg = 0 and with field_cg = 1, 2, 3.  Prints per run "run K cg_kernel iterations" and every displacement as a hexadecimal
// double, for the test to compare.
#include <cmath>
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
    std::vector<Node> posed;
    for (std::size_t i = 0; ok && i < N; ++i) {
        double x, y, ux, uy, fx, fy;
        int kx, ky;
        ok = std::fscanf(in, "%la %la %d %d %la %la %la %la", &x, &y, &kx, &ky, &ux, &uy, &fx, &fy) == 8;
        Node n{{x, y}, std::nullopt, std::nullopt, std::nullopt, std::nullopt};
        if (kx) n.ux = ux; else n.fx = fx;
        if (ky) n.uy = uy; else n.fy = fy;
        posed.push_back(n);
    }
    std::vector<Element> elements;
    for (std::size_t e = 0; ok && e < E; ++e) {
        std::size_t a, b, c;
        ok = std::fscanf(in, "%zu %zu %zu", &a, &b, &c) == 3;
        elements.push_back({{a, b, c}, std::nullopt});
    }
    std::vector<double> scale(E);
    for (std::size_t e = 0; ok && e < E; ++e) ok = std::fscanf(in, "%la", &scale[e]) == 1;
    std::fclose(in);
    if (!ok) {
        std::printf("FAIL the problem file does not parse\n");
        return 2;
    }
    mag_options opt;
    mag_default_options(&opt);
    ok = ok && opt.field_cg == 0;
    opt.stop_mode = MAG_STOP_REL;
    opt.tol = 1e-12;
    for (int kind = 0; kind <= 3; ++kind) {
        opt.field_cg = kind;
        std::vector<Node> nodes = posed;
        std::vector<Element> els = elements;
        FieldSession session;
        mag_stats st{};
        if (Result e = solver::set_element_scale(session, nodes, els, meta, scale, &opt, &st)) {
            std::printf("FAIL %s\n", e->display().c_str());
            return 2;
        }
        ok = ok && st.cg_kernel == (kind == 0 ? 3 : 5) && st.converged == 1;
        std::printf("run %d %d %lld\n", kind, (int)st.cg_kernel, (long long)st.iterations);
        for (std::size_t i = 0; i < N; ++i) std::printf("u %d %zu %a %a\n", kind, i, *nodes[i].ux, *nodes[i].uy);
    }
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
