// Compiled-caller check of solver::refine and solver::upload_refined (include/magnetite_solver.hpp) on the problem in the file it
// is given (written by tests/test_refine_cpp.py from the tensile fixture: "N E youngs nu t", then per node "x y known_x known_y ux
// uy fx fy", then per element its three nodes; floats hexadecimal).  Refines the solved part by its ZZ indicator with either
// split, and by marks without a solve, and writes every array of every result raw into the directory given second, for the test
// to compare bit for bit with the Python binding's; then the adaptive loop of two rounds, one line per solve.
#include <cstdio>
#include <string>

#include "magnetite_solver.hpp"

using namespace magnetite;

template <class T>
static bool dump(const std::string &path, const std::vector<T> &v)
{
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

// the refined part as the arrays of mag_download_refine
static bool dump(const std::string &dir, const char *tag, const Refined &r)
{
    std::vector<double> xy, u_in, f_in;
    std::vector<std::uint8_t> known;
    std::vector<std::int32_t> conn;
    for (const Node &n : r.nodes) {
        xy.push_back(n.vertex.x);
        xy.push_back(n.vertex.y);
        known.push_back(n.ux.has_value());
        known.push_back(n.uy.has_value());
        u_in.push_back(n.ux.value_or(0.0));
        u_in.push_back(n.uy.value_or(0.0));
        f_in.push_back(n.fx.value_or(0.0));
        f_in.push_back(n.fy.value_or(0.0));
        if (n.ux.has_value() == n.fx.has_value() || n.uy.has_value() == n.fy.has_value()) return false;
    }
    for (const Element &e : r.elements)
        for (std::size_t n : e.nodes) conn.push_back((std::int32_t)n);
    const std::string base = dir + "/" + tag + "_";
    std::printf("%s nodes %zu elements %zu marked %lld marked_edges %lld sweeps %lld split %lld %lld %lld\n", tag, r.nodes.size(), r.elements.size(),
                (long long)r.marked, (long long)r.marked_edges, (long long)r.sweeps, (long long)r.split2, (long long)r.split3, (long long)r.split4);
    return dump(base + "xy.bin", xy) && dump(base + "conn.bin", conn) && dump(base + "u_known.bin", known) && dump(base + "u_in.bin", u_in) &&
           dump(base + "f_in.bin", f_in) && dump(base + "node_parents.bin", r.node_parents) && dump(base + "elem_parent.bin", r.elem_parent);
}

int main(int argc, char **argv)
{
    std::FILE *in = argc > 2 ? std::fopen(argv[1], "r") : nullptr;
    if (!in) {
        std::printf("FAIL no problem file or no output directory\n");
        return 2;
    }
    const std::string dir = argv[2];
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
    Refined out;
    RefineSpec spec;  // the defaults: the fifth of the elements with the largest ZZ indicator, their longest edges
    if (Result e = solver::refine(nodes, elements, meta, spec, out)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ok && dump(dir, "top1", out);
    spec.split = 3;
    spec.rule = MAG_REFINE_MAX_FRACTION;
    spec.theta = 0.5;
    if (Result e = solver::refine(nodes, elements, meta, spec, out)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ok && dump(dir, "max3", out);
    RefineSpec by_marks;
    by_marks.marks.assign(E, 0);
    for (std::size_t e = 0; e < E; e += 7) by_marks.marks[e] = 1;
    if (Result e = solver::refine(nodes, elements, meta, by_marks, out)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    ok = ok && dump(dir, "marks1", out) && out.elem_parent.size() == out.elements.size() && 2 * (out.nodes.size() - N) == out.node_parents.size();
    // arguments the library refuses are errors, not crashes
    RefineSpec bad;
    bad.theta = 0.0;
    Result e2 = solver::refine(nodes, elements, meta, bad, out);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    bad = RefineSpec{};
    bad.marks.assign(E + 1, 1);
    e2 = solver::refine(nodes, elements, meta, bad, out);
    ok = ok && e2.has_value() && e2->display().rfind("Solver error:", 0) == 0;
    // the adaptive loop
    std::vector<AdaptRound> history;
    std::vector<Node> adapted = nodes, posed;
    std::vector<Element> adapted_elements = elements;
    if (Result e = solver::upload_refined(adapted, adapted_elements, meta, RefineSpec{}, 2, history, nullptr, &posed)) {
        std::printf("FAIL %s\n", e->display().c_str());
        return 2;
    }
    for (std::size_t r = 0; r < history.size(); ++r)
        std::printf("adapt %zu nodes %zu elements %zu eta %a eta_rel %a iterations %lld\n", r, history[r].nodes, history[r].elements, history[r].eta,
                    history[r].eta_rel, (long long)history[r].iterations);
    ok = ok && history.size() == 3 && adapted.size() == history[2].nodes && adapted_elements.size() == history[2].elements && posed.size() == adapted.size();
    std::vector<double> u;
    for (const Node &n : adapted) {
        ok = ok && n.ux && n.uy && n.fx && n.fy;
        u.push_back(n.ux.value_or(0.0));
        u.push_back(n.uy.value_or(0.0));
    }
    for (const Element &e : adapted_elements) ok = ok && e.stress.has_value();
    Refined last;
    last.nodes = posed;
    last.elements = adapted_elements;
    ok = ok && dump(dir, "adapt2", last) && dump(dir + "/adapt2_u.bin", u);
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
