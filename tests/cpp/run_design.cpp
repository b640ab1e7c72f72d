// Compiled-caller check of solver::design_init, design_step, design_info, download_design and set_element_scale
// (include/magnetite_solver.hpp) on the problem in the file it is given (written by tests/test_design_cpp.py from plate(6, 5):
// "N E youngs nu t", then per node "x y known_x known_y ux uy fx fy", then per element its three nodes; floats hexadecimal).
// Three iterations of the design loop; prints every result as a hexadecimal double, for the test to compare bit for bit with the
// Python binding's.
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
    mag_options opt;
    mag_default_options(&opt);
    opt.stop_mode = MAG_STOP_REL;
    opt.tol = 1e-10;
    FieldSession session;
    DesignSpec spec;
    if (Result e = solver::design_init(session, nodes, elements, meta, spec, &opt)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    for (int k = 0; k < 3; ++k) {
        DesignInfo info;
        mag_stats st{};
        if (Result e = solver::design_step(session, &info, &st)) {
            std::printf("FAIL %s\n", e->display().c_str());
            return 2;
        }
        ok = ok && info.steps == k + 1 && st.cg_kernel == 3;
        std::printf("step %d %a %a %a %a %a %d %lld\n", k, info.J, info.volume_fraction, info.lagrange, info.change, info.greyness,
                    info.reachable ? 1 : 0, (long long)st.iterations);
    }
    Design d;
    if (Result e = solver::download_design(session, d)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ok && d.rho.size() == E && d.rho_filtered.size() == E && d.scale.size() == E && d.dJ_drho.size() == E;
    for (std::size_t e = 0; ok && e < E; ++e) std::printf("element %zu %a %a %a %a\n", e, d.rho[e], d.rho_filtered[e], d.scale[e], d.dJ_drho[e]);
    // the final design's scale as a field of the caller's: the part solved under it (which fills every value of `nodes` in)
    const std::vector<Node> posed = nodes;
    FieldSession solved;
    mag_stats st{};
    if (Result e = solver::set_element_scale(solved, nodes, elements, meta, d.scale, &opt, &st)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ok && st.cg_kernel == 3;
    double sum = 0.0;
    for (const Node &n : nodes) sum += *n.ux + *n.uy;
    std::printf("solved %a %lld\n", sum, (long long)st.iterations);
    // what the library refuses is an error, not a crash
    spec.penal = 0;
    Result e2 = solver::design_init(session, posed, elements, meta, spec, &opt);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    std::vector<double> bad(E, 1.0);
    bad[3] = -1.0;
    std::vector<Node> again = posed;
    Result e3 = solver::set_element_scale(solved, again, elements, meta, bad, &opt);
    ok = ok && e2->display().find("penal") != std::string::npos && e3.has_value() && e3->display().find("scale[3]") != std::string::npos;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
