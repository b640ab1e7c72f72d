// magnetite_gpu -- compiled caller with the stage order of the reference's entry() (main.rs:54-76):
//     mesher (input JSON + boundary rules; the mesh itself comes pre-generated as a Gmsh MSH-4 ASCII file, because
//     the reference's `gmsh` subprocess, mesher.rs:501-506, is outside the hot path) -> solver::run -> csv_output.
// Everything numerical happens in libmagnetite_hip.so through include/magnetite_solver.hpp; this file is glue:
//   * input JSON            mesher.rs:713-808   (tiny order-preserving JSON reader below; no third-party library)
//   * boundary rules        mesher.rs:815-930   strict region test, every matching rule overwrites, later rules win
//   * MSH-4 ASCII           mesher.rs:536-704   + check_ccw with its `< 1.0` quirk (mesher.rs:522-526)
//   * nodes.csv/elements.csv post_processor.rs:18-83, floats as Rust's `{}` prints them
// Usage: magnetite_gpu <input.json> <mesh.msh> [--nodes nodes.csv] [--elements elements.csv] [--dry-run] [--rel TOL]
//                      [--stress-recovery] [--modal P --density RHO] [--buckling P [--subspace Q]] [--adapt R [--refine-fraction T] [--refine-split 1|3]]
//                      [--transient STEPS --dt DT --density RHO [--rayleigh A,E] [--probe DOF]... [--kinematics linear|tl [--newton-tol T]]]
//                      [--explicit STEPS --density RHO [--dt DT | --dt-scale S] [--rayleigh A,E] [--probe DOF]... [--record-every K]
//                       [--kinematics linear|tl]]
//                      [--nonlinear INCREMENTS [--newton-tol T] [--line-search H] [--probe DOF]...]
//                      [--material svk|neo-hooke]
//   --dry-run  stop before the solver and print what was parsed (no GPU needed)
//   --rel TOL  stop CG on relative residual TOL instead of the reference's absolute 1e-4
//   --buckling P [--subspace Q]  after the linear solve, also print "info: buckling mode k load factor L residual R" for the P load
//              factors of smallest magnitude under the input's own loads (negative: buckling under the reversed load) and write
//              buckling_modes.csv (id,ux1,uy1,...,uxP,uyP) next to nodes.csv -- solver::buckling
//   --modal P --density RHO  also print "info: mode k frequency F Hz residual R" for the P lowest modes and write modes.csv
//              (id,ux1,uy1,...,uxP,uyP) next to nodes.csv -- solver::modal; the input JSON has no density, hence the flag
//   --transient STEPS --dt DT --density RHO  also run STEPS steps of Newmark's method from rest under the loads applied at t = 0
//              (solver::transient; --rayleigh A,E: C = A M + E K), print "info: step n t T iterations I" per step and write
//              history.csv (step,t, then u,v,a per --probe DOF, DOF = 2 * node + axis) next to nodes.csv; --kinematics tl: every step
//              by Newton's method on the total-Lagrangian tangent (solver::transient_tl: large rotations at an implicit step;
//              --rayleigh A,0 only; --newton-tol T), prints "info: transient kinematics total-lagrangian", then "info: step n t T
//              newton I iterations C" per step, "warning: transient: ..." when a step did not converge (the rows end at the last
//              converged step) or an element was inverted
//   --explicit STEPS --density RHO  also run STEPS central-difference steps on the lumped mass from rest under the loads applied at
//              t = 0 (solver::run_explicit: one fused launch a step; --dt DT, or --dt-scale S times the device's bound of the
//              stable step, 0.9 by default), print "info: explicit dt D (bound B)" and "info: step n t T" per recorded row
//              (--record-every K: steps 0, K, 2K, ...) and write history.csv as --transient does; --kinematics tl: the
//              total-Lagrangian internal force in place of K u (large rotations; --rayleigh A,0 only), prints "info: explicit
//              kinematics total-lagrangian" and "warning: explicit: an element was inverted (det F <= 0)" when one was
//   --nonlinear INCREMENTS  solve the large-deflection equilibrium under the total-Lagrangian internal force in INCREMENTS load
//              increments of Newton's method (solver::run_newton; --newton-tol T, --line-search H), print "info: increment k load L
//              newton I cg C residual R" per converged increment, write nodes.csv / elements.csv from the NONLINEAR result (u; the
//              von Mises value of the second Piola-Kirchhoff stress) and load_path.csv (increment,load,newton,W,Pi, then u per
//              --probe DOF) next to nodes.csv
//   --material svk|neo-hooke  the material law of the total-Lagrangian passes (solver::set_material_law): with --nonlinear, or with
//              --explicit / --transient under --kinematics tl; prints "info: material neo-hooke".  Refused with the linear passes
//   --stress-recovery  also write nodes_stress.csv (id,sx,sy,txy,vm) and elements_stress.csv (id,sx,sy,txy,vm,eta2) next to the
//              two files -- solver::stress_recovery: the tensor per element, the nodal field, the ZZ error indicator -- and
//              print eta_rel; without it nothing changes
//   --adapt R  the adaptive loop of solver::upload_refined instead of the one solve: R times solve -> stress recovery -> refine
//              the T (default 0.2) of the elements with the largest ZZ indicator by longest-edge bisection (--refine-split 3:
//              all three edges of a marked element) -> upload, on the device, then the final solve; prints "info: adapt round r:
//              N nodes, E elements, eta_rel X" per solve, and the two files (and what the other flags write) are the FINAL
//              mesh's; without it nothing changes
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "magnetite_solver.hpp"

using namespace magnetite;

namespace {

[[noreturn]] void die(const MagnetiteError &e)
{
    std::fprintf(stderr, "Received error: %s\n", e.display().c_str());  // main.rs:44-50
    std::exit(1);
}

// ---- order-preserving JSON (objects keep the file's key order: boundary rules apply in that order) ----
struct Json {
    enum Kind { Null, Bool, Num, Str, Arr, Obj } kind = Null;
    double num = 0.0;
    bool b = false;
    std::string str;
    std::vector<Json> arr;
    std::vector<std::pair<std::string, Json>> obj;
    const Json *get(const std::string &k) const
    {
        for (const auto &kv : obj)
            if (kv.first == k) return &kv.second;
        return nullptr;
    }
    bool has(const std::string &k) const { return get(k) != nullptr; }
    std::optional<double> as_f64() const { return kind == Num ? std::optional<double>(num) : std::nullopt; }
};

struct JsonParser {
    const std::string &s;
    size_t i = 0;
    explicit JsonParser(const std::string &text) : s(text) {}
    void ws()
    {
        while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\t' || s[i] == '\r')) ++i;
    }
    [[noreturn]] void bad(const char *what) { die({MagnetiteError::Input, std::string("Error in input file json: ") + what}); }
    Json value()
    {
        ws();
        if (i >= s.size()) bad("unexpected end");
        Json v;
        const char c = s[i];
        if (c == '{') {
            v.kind = Json::Obj;
            ++i;
            ws();
            if (i < s.size() && s[i] == '}') { ++i; return v; }
            for (;;) {
                ws();
                Json key = value();
                if (key.kind != Json::Str) bad("object key is not a string");
                ws();
                if (i >= s.size() || s[i] != ':') bad("expected ':'");
                ++i;
                v.obj.emplace_back(key.str, value());
                ws();
                if (i < s.size() && s[i] == ',') { ++i; continue; }
                if (i < s.size() && s[i] == '}') { ++i; break; }
                bad("expected ',' or '}'");
            }
        } else if (c == '[') {
            v.kind = Json::Arr;
            ++i;
            ws();
            if (i < s.size() && s[i] == ']') { ++i; return v; }
            for (;;) {
                v.arr.push_back(value());
                ws();
                if (i < s.size() && s[i] == ',') { ++i; continue; }
                if (i < s.size() && s[i] == ']') { ++i; break; }
                bad("expected ',' or ']'");
            }
        } else if (c == '"') {
            v.kind = Json::Str;
            ++i;
            while (i < s.size() && s[i] != '"') {
                if (s[i] == '\\' && i + 1 < s.size()) ++i;
                v.str.push_back(s[i++]);
            }
            if (i >= s.size()) bad("unterminated string");
            ++i;
        } else if (!s.compare(i, 4, "null")) {
            i += 4;
        } else if (!s.compare(i, 4, "true")) {
            v.kind = Json::Bool;
            v.b = true;
            i += 4;
        } else if (!s.compare(i, 5, "false")) {
            v.kind = Json::Bool;
            i += 5;
        } else {
            char *end = nullptr;
            v.num = std::strtod(s.c_str() + i, &end);
            if (end == s.c_str() + i) bad("unexpected character");
            v.kind = Json::Num;
            i = (size_t)(end - s.c_str());
        }
        return v;
    }
};

std::string slurp(const std::string &path, MagnetiteError::Kind kind, const std::string &msg)
{
    std::ifstream f(path);
    if (!f) die({kind, msg});
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// ---- datatypes.rs:31-52 ----
struct BoundaryRule {
    std::string name;
    double x_min = std::numeric_limits<double>::lowest(), x_max = std::numeric_limits<double>::max();
    double y_min = std::numeric_limits<double>::lowest(), y_max = std::numeric_limits<double>::max();
    std::optional<double> ux, uy, fx, fy;
};

// mesher.rs:769-808
ModelMetadata parse_input_metadata(const Json &doc)
{
    const Json *md = doc.get("metadata");
    auto f = [&](const char *k) { return md && md->get(k) ? md->get(k)->as_f64() : std::nullopt; };
    const auto e = f("material_elasticity"), t = f("part_thickness"), nu = f("poisson_ratio");
    const auto cmin = f("characteristic_length_min"), cmax = f("characteristic_length_max");
    if (!e) die({MagnetiteError::Input, "Input json missing material elasticity"});
    if (!nu) die({MagnetiteError::Input, "Input json missing poisson ratio"});
    if (!cmin) die({MagnetiteError::Input, "Input json missing minimum characteristic length"});
    if (!cmax) die({MagnetiteError::Input, "Input json missing maximum characteristic length"});
    if (!t) die({MagnetiteError::Input, "Input json missing part thickness"});  // the reference unwrap()-panics
    return ModelMetadata{*e, *nu, *t, (float)*cmin, (float)*cmax};
}

// mesher.rs:822-904
std::vector<BoundaryRule> parse_boundary_rules(const Json &doc)
{
    std::vector<BoundaryRule> rules;
    const Json *bc = doc.get("boundary_conditions");
    if (!bc) return rules;
    for (const auto &kv : bc->obj) {
        const std::string &name = kv.first;
        const Json &rj = kv.second;
        if (!rj.has("region")) die({MagnetiteError::Input, "Boundary rule " + name + " is missing region field"});
        if (!rj.has("targets")) die({MagnetiteError::Input, "Boundary rule " + name + " is missing target field"});
        BoundaryRule r;
        r.name = name;
        const Json &reg = *rj.get("region"), &tg = *rj.get("targets");
        auto bound = [&](const char *k, double &dst) {
            if (!reg.has(k)) return;
            const auto v = reg.get(k)->as_f64();
            if (!v) die({MagnetiteError::Input, std::string("Bad value for ") + k + " in " + name});
            dst = *v;
        };
        bound("x_target_min", r.x_min);
        bound("x_target_max", r.x_max);
        bound("y_target_min", r.y_min);
        bound("y_target_max", r.y_max);
        auto target = [&](const char *k) { return tg.get(k) ? tg.get(k)->as_f64() : std::nullopt; };
        r.ux = target("ux");
        r.uy = target("uy");
        r.fx = target("fx");
        r.fy = target("fy");
        const std::string b = "Boundary '" + name + "' ";
        if (r.x_min > r.x_max) die({MagnetiteError::Input, b + "has x_target_min greater than x_target_max"});
        if (r.y_min > r.y_max) die({MagnetiteError::Input, b + "has y_target_min greater than y_target_max"});
        if (!r.fx && !r.ux) die({MagnetiteError::Input, b + "is under-constrained in x-axis"});
        if (!r.fy && !r.uy) die({MagnetiteError::Input, b + "is under-constrained in y-axis"});
        if (r.fx && r.ux) die({MagnetiteError::Input, b + "is over-constrained in x-axis"});
        if (r.fy && r.uy) die({MagnetiteError::Input, b + "is over-constrained in y-axis"});
        rules.push_back(r);
    }
    std::printf("info: loaded %zu boundary rules from input file\n", rules.size());
    return rules;
}

// mesher.rs:913-927
void apply_boundary_conditions(const std::vector<BoundaryRule> &rules, std::vector<Node> &nodes)
{
    for (Node &n : nodes)
        for (const BoundaryRule &r : rules) {
            const bool candidate = n.vertex.x > r.x_min && n.vertex.x < r.x_max && n.vertex.y > r.y_min && n.vertex.y < r.y_max;
            if (candidate) {
                n.ux = r.ux;
                n.uy = r.uy;
                n.fx = r.fx;
                n.fy = r.fy;
            }
        }
}

// mesher.rs:536-704 (+ check_ccw, :522-526)
void parse_mesh(const std::string &path, std::vector<Node> &nodes, std::vector<Element> &elements)
{
    std::ifstream f(path);
    if (!f) die({MagnetiteError::Mesher, "Unable to open auto-generated mesh file: " + path});
    enum { Limbo, Entities, Nodes, Elements } state = Limbo;
    bool skipped_meta = false;
    std::vector<std::pair<size_t, Node>> unordered;
    std::string line;
    auto ints = [&](const std::string &l) {
        std::vector<long long> v;
        std::stringstream ss(l);
        long long x;
        while (ss >> x) v.push_back(x);
        if (v.empty()) die({MagnetiteError::Mesher, "Unexpected non-int in mesh data " + l});
        return v;
    };
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (line.rfind("$End", 0) == 0) state = Limbo;
        if (state == Limbo) {
            skipped_meta = false;
            if (line.rfind("$Entities", 0) == 0) state = Entities;
            else if (line.rfind("$Node", 0) == 0) state = Nodes;
            else if (line.rfind("$Elements", 0) == 0) state = Elements;
            continue;
        }
        if (state == Entities) continue;
        if (!skipped_meta) { skipped_meta = true; continue; }
        const auto head = ints(line);
        if (head.size() < 4) die({MagnetiteError::Mesher, "short block header in mesh data"});
        if (state == Nodes) {
            const size_t n_local = (size_t)head[3];
            std::vector<size_t> tags(n_local);
            for (size_t k = 0; k < n_local; ++k) {
                if (!std::getline(f, line)) die({MagnetiteError::Mesher, "truncated node block"});
                tags[k] = (size_t)std::stoll(line);
            }
            for (size_t k = 0; k < n_local; ++k) {
                if (!std::getline(f, line)) die({MagnetiteError::Mesher, "truncated node block"});
                std::stringstream ss(line);
                double x = 0, y = 0;
                ss >> x >> y;
                unordered.push_back({tags[k] - 1, Node{{x, y}, std::nullopt, std::nullopt, 0.0, 0.0}});  // mesher.rs:615-624
            }
        } else {
            const long long entity_dim = head[0];
            const size_t n_local = (size_t)head[3];
            for (size_t k = 0; k < n_local; ++k) {
                if (!std::getline(f, line)) die({MagnetiteError::Mesher, "truncated element block"});
                if (entity_dim != 2) continue;
                const auto md = ints(line);
                if (md.size() < 4) die({MagnetiteError::Mesher, "element with fewer than 3 nodes"});
                elements.push_back({{(size_t)md[1] - 1, (size_t)md[2] - 1, (size_t)md[3] - 1}, std::nullopt});
            }
        }
    }
    nodes.assign(unordered.size(), Node{{0, 0}, std::nullopt, std::nullopt, 0.0, 0.0});
    for (auto &kv : unordered) {
        if (kv.first >= nodes.size()) die({MagnetiteError::Mesher, "node tags are not a permutation of 1..N"});
        nodes[kv.first] = kv.second;
    }
    for (Element &e : elements) {
        for (size_t n : e.nodes)
            if (n >= nodes.size()) die({MagnetiteError::Mesher, "element references a node outside the mesh"});
        if (solver::compute_element_area(e, nodes) < 1.0) std::swap(e.nodes[0], e.nodes[2]);  // check_ccw: reverse()
    }
    std::printf("info: loaded %zu nodes and %zu elements\n", nodes.size(), elements.size());
}

// Rust's `{}` for f64: shortest representation that round-trips, never in exponent form, no trailing ".0"
std::string rust_display(double v)
{
    if (v != v) return "NaN";
    if (v == std::numeric_limits<double>::infinity()) return "inf";
    if (v == -std::numeric_limits<double>::infinity()) return "-inf";
    char buf[512];
    const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

// post_processor.rs:18-83
void csv_output(const std::vector<Element> &elements, const std::vector<Node> &nodes, const std::string &nodes_output,
                const std::string &elements_output)
{
    std::FILE *nf = std::fopen(nodes_output.c_str(), "w");
    if (!nf) die({MagnetiteError::Solver, "Failed to create nodes.csv: " + nodes_output});
    std::FILE *ef = std::fopen(elements_output.c_str(), "w");
    if (!ef) die({MagnetiteError::Solver, "Failed to create elements.csv: " + elements_output});
    std::fputs("x,y,ux,uy\n", nf);
    for (const Node &n : nodes)
        std::fprintf(nf, "%s,%s,%s,%s\n", rust_display(n.vertex.x).c_str(), rust_display(n.vertex.y).c_str(),
                     rust_display(n.ux.value()).c_str(), rust_display(n.uy.value()).c_str());
    std::fputs("n0,n1,n2,stress\n", ef);
    for (const Element &e : elements)
        std::fprintf(ef, "%zu,%zu,%zu,%s\n", e.nodes[0], e.nodes[1], e.nodes[2], rust_display(e.stress.value()).c_str());
    std::fclose(nf);
    std::fclose(ef);
    std::printf("info: wrote output to %s and %s\n", nodes_output.c_str(), elements_output.c_str());
}

// "dir/nodes.csv" -> "dir/nodes_stress.csv"
std::string stress_name(const std::string &path)
{
    const size_t slash = path.find_last_of('/'), dot = path.find_last_of('.');
    const bool ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
    return ext ? path.substr(0, dot) + "_stress" + path.substr(dot) : path + "_stress";
}

// the rows of solver::stress_recovery, floats as csv_output prints them
void stress_output(const StressField &s, const std::string &nodes_output, const std::string &elements_output)
{
    std::FILE *nf = std::fopen(nodes_output.c_str(), "w");
    if (!nf) die({MagnetiteError::Solver, "Failed to create nodes_stress.csv: " + nodes_output});
    std::FILE *ef = std::fopen(elements_output.c_str(), "w");
    if (!ef) die({MagnetiteError::Solver, "Failed to create elements_stress.csv: " + elements_output});
    std::fputs("id,sx,sy,txy,vm\n", nf);
    for (size_t i = 0; 4 * i < s.node.size(); ++i)
        std::fprintf(nf, "%zu,%s,%s,%s,%s\n", i, rust_display(s.node[4 * i]).c_str(), rust_display(s.node[4 * i + 1]).c_str(),
                     rust_display(s.node[4 * i + 2]).c_str(), rust_display(s.node[4 * i + 3]).c_str());
    std::fputs("id,sx,sy,txy,vm,eta2\n", ef);
    for (size_t e = 0; e < s.eta2.size(); ++e)
        std::fprintf(ef, "%zu,%s,%s,%s,%s,%s\n", e, rust_display(s.elem[4 * e]).c_str(), rust_display(s.elem[4 * e + 1]).c_str(),
                     rust_display(s.elem[4 * e + 2]).c_str(), rust_display(s.elem[4 * e + 3]).c_str(), rust_display(s.eta2[e]).c_str());
    std::fclose(nf);
    std::fclose(ef);
    std::printf("info: wrote stress recovery to %s and %s\n", nodes_output.c_str(), elements_output.c_str());
}

// "dir/nodes.csv" -> "dir/modes.csv"
std::string modes_name(const std::string &nodes_output)
{
    const size_t slash = nodes_output.find_last_of('/');
    return (slash == std::string::npos ? std::string() : nodes_output.substr(0, slash + 1)) + "modes.csv";
}

// "dir/nodes.csv" -> "dir/buckling_modes.csv"
std::string buckling_modes_name(const std::string &nodes_output)
{
    const size_t slash = nodes_output.find_last_of('/');
    return (slash == std::string::npos ? std::string() : nodes_output.substr(0, slash + 1)) + "buckling_modes.csv";
}

// P shapes of solver::modal or solver::buckling, a row per node, floats as csv_output prints them
void shapes_output(const std::vector<double> &shapes, size_t P, size_t num_nodes, const std::string &path, const char *what)
{
    std::FILE *mf = std::fopen(path.c_str(), "w");
    if (!mf) die({MagnetiteError::Solver, "Failed to create " + path});
    std::fputs("id", mf);
    for (size_t k = 1; k <= P; ++k) std::fprintf(mf, ",ux%zu,uy%zu", k, k);
    std::fputs("\n", mf);
    for (size_t i = 0; i < num_nodes; ++i) {
        std::fprintf(mf, "%zu", i);
        for (size_t k = 0; k < P; ++k)
            std::fprintf(mf, ",%s,%s", rust_display(shapes[k * 2 * num_nodes + 2 * i]).c_str(),
                         rust_display(shapes[k * 2 * num_nodes + 2 * i + 1]).c_str());
        std::fputs("\n", mf);
    }
    std::fclose(mf);
    std::printf("info: wrote %s to %s\n", what, path.c_str());
}

void modes_output(const Modes &m, size_t num_nodes, const std::string &path)
{
    shapes_output(m.shapes, m.lambda.size(), num_nodes, path, "mode shapes");
}

// "dir/nodes.csv" -> "dir/history.csv"
std::string history_name(const std::string &nodes_output)
{
    const size_t slash = nodes_output.find_last_of('/');
    return (slash == std::string::npos ? std::string() : nodes_output.substr(0, slash + 1)) + "history.csv";
}

// the probes' rows of solver::transient, a row per step, floats as csv_output prints them
void history_output(const std::vector<double> &time, const std::vector<std::size_t> &step, const std::vector<double> &probe_u,
                    const std::vector<double> &probe_v, const std::vector<double> &probe_a, const std::vector<std::int32_t> &probes,
                    const std::string &path);
void history_output(const Transient &tr, const std::vector<std::int32_t> &probes, double dt, const std::string &path)
{
    std::vector<double> time;
    std::vector<std::size_t> step;
    for (size_t n = 0; n < tr.iterations.size(); ++n) time.push_back((double)n * dt), step.push_back(n);
    history_output(time, step, tr.probe_u, tr.probe_v, tr.probe_a, probes, path);
}

// a row per recorded step (solver::transient: every step; solver::run_explicit: steps 0, record_every, ...)
void history_output(const std::vector<double> &time, const std::vector<std::size_t> &step, const std::vector<double> &probe_u,
                    const std::vector<double> &probe_v, const std::vector<double> &probe_a, const std::vector<std::int32_t> &probes,
                    const std::string &path)
{
    std::FILE *hf = std::fopen(path.c_str(), "w");
    if (!hf) die({MagnetiteError::Solver, "Failed to create history.csv: " + path});
    std::fputs("step,t", hf);
    for (std::int32_t d : probes) std::fprintf(hf, ",u%d,v%d,a%d", (int)d, (int)d, (int)d);
    std::fputs("\n", hf);
    const size_t P = probes.size();
    for (size_t n = 0; n < time.size(); ++n) {
        std::fprintf(hf, "%zu,%s", step[n], rust_display(time[n]).c_str());
        for (size_t k = 0; k < P; ++k)
            std::fprintf(hf, ",%s,%s,%s", rust_display(probe_u[n * P + k]).c_str(), rust_display(probe_v[n * P + k]).c_str(),
                         rust_display(probe_a[n * P + k]).c_str());
        std::fputs("\n", hf);
    }
    std::fclose(hf);
    std::printf("info: wrote the probes' history to %s\n", path.c_str());
}

// "dir/nodes.csv" -> "dir/load_path.csv"
std::string load_path_name(const std::string &nodes_output)
{
    const size_t slash = nodes_output.find_last_of('/');
    return (slash == std::string::npos ? std::string() : nodes_output.substr(0, slash + 1)) + "load_path.csv";
}

// the load-deflection curve of solver::run_newton, a row per converged increment behind the start's, floats as csv_output prints them
void load_path_output(const Newton &nl, const std::vector<std::int32_t> &probes, const std::string &path)
{
    std::FILE *lf = std::fopen(path.c_str(), "w");
    if (!lf) die({MagnetiteError::Solver, "Failed to create load_path.csv: " + path});
    std::fputs("increment,load,newton,W,Pi", lf);
    for (std::int32_t d : probes) std::fprintf(lf, ",u%d", (int)d);
    std::fputs("\n", lf);
    const size_t P = probes.size();
    for (size_t k = 0; k <= (size_t)nl.increments_converged; ++k) {
        std::fprintf(lf, "%zu,%s,%d,%s,%s", k, rust_display(nl.load[k]).c_str(), (int)nl.newton_iterations[k], rust_display(nl.energies[2 * k]).c_str(),
                     rust_display(nl.energies[2 * k + 1]).c_str());
        for (size_t j = 0; j < P; ++j) std::fprintf(lf, ",%s", rust_display(nl.probe_u[k * P + j]).c_str());
        std::fputs("\n", lf);
    }
    std::fclose(lf);
    std::printf("info: wrote the load path to %s\n", path.c_str());
}

// "dir/elements.csv" -> "dir/density.csv"
std::string density_name(const std::string &elements_output)
{
    const size_t slash = elements_output.find_last_of('/');
    return (slash == std::string::npos ? std::string() : elements_output.substr(0, slash + 1)) + "density.csv";
}

// the design of solver::download_design, a row per element, floats as csv_output prints them
void density_output(const Design &d, const std::string &path)
{
    std::FILE *df = std::fopen(path.c_str(), "w");
    if (!df) die({MagnetiteError::Solver, "Failed to create density.csv: " + path});
    std::fputs("element,rho,rho_filtered,scale\n", df);
    for (size_t e = 0; e < d.rho.size(); ++e)
        std::fprintf(df, "%zu,%s,%s,%s\n", e, rust_display(d.rho[e]).c_str(), rust_display(d.rho_filtered[e]).c_str(),
                     rust_display(d.scale[e]).c_str());
    std::fclose(df);
    std::printf("info: wrote the design to %s\n", path.c_str());
}

}  // namespace

int main(int argc, char **argv)
{
    std::string input, mesh, nodes_out = "nodes.csv", elements_out = "elements.csv";
    bool dry = false, recover = false;
    int modal_modes = 0, buckling_modes = 0, buckling_subspace = 0, adapt = 0, refine_split = 1, topopt = 0, penal = 3, filter_passes = 1, field_cg = 0, transient_steps = 0;
    double rel = 0.0, density = 0.0, refine_fraction = 0.2, volume_fraction = 0.5, dt = 0.0, rayleigh_mass = 0.0, rayleigh_stiffness = 0.0;
    bool transient = false, explicit_run = false;
    int nonlinear = -1, line_search = 0;
    double newton_tol = 0.0;
    int explicit_steps = 0, record_every = 1;
    double dt_scale = 0.0;
    std::string kinematics, material;
    std::vector<std::int32_t> probes;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--dry-run") dry = true;
        else if (a == "--stress-recovery") recover = true;
        else if (a == "--modal" && i + 1 < argc) modal_modes = std::atoi(argv[++i]);
        else if (a == "--buckling" && i + 1 < argc) buckling_modes = std::atoi(argv[++i]);
        else if (a == "--subspace" && i + 1 < argc) buckling_subspace = std::atoi(argv[++i]);
        else if (a == "--density" && i + 1 < argc) density = std::atof(argv[++i]);
        else if (a == "--transient" && i + 1 < argc) transient = true, transient_steps = std::atoi(argv[++i]);
        else if (a == "--dt" && i + 1 < argc) dt = std::atof(argv[++i]);
        else if (a == "--explicit" && i + 1 < argc) explicit_run = true, explicit_steps = std::atoi(argv[++i]);
        else if (a == "--dt-scale" && i + 1 < argc) dt_scale = std::atof(argv[++i]);
        else if (a == "--record-every" && i + 1 < argc) record_every = std::atoi(argv[++i]);
        else if (a == "--kinematics" && i + 1 < argc) kinematics = argv[++i];
        else if (a == "--material" && i + 1 < argc) material = argv[++i];
        else if (a == "--nonlinear" && i + 1 < argc) nonlinear = std::atoi(argv[++i]);
        else if (a == "--newton-tol" && i + 1 < argc) newton_tol = std::atof(argv[++i]);
        else if (a == "--line-search" && i + 1 < argc) line_search = std::atoi(argv[++i]);
        else if (a == "--probe" && i + 1 < argc) probes.push_back((std::int32_t)std::atoi(argv[++i]));
        else if (a == "--rayleigh" && i + 1 < argc) {
            const std::string pair = argv[++i];
            const size_t comma = pair.find(',');
            if (comma == std::string::npos) die({MagnetiteError::Input, "--rayleigh A,E needs two values"});
            rayleigh_mass = std::atof(pair.substr(0, comma).c_str());
            rayleigh_stiffness = std::atof(pair.substr(comma + 1).c_str());
        }
        else if (a == "--adapt" && i + 1 < argc) adapt = std::atoi(argv[++i]);
        else if (a == "--refine-fraction" && i + 1 < argc) refine_fraction = std::atof(argv[++i]);
        else if (a == "--refine-split" && i + 1 < argc) refine_split = std::atoi(argv[++i]);
        else if (a == "--topopt" && i + 1 < argc) topopt = std::atoi(argv[++i]);
        else if (a == "--volume-fraction" && i + 1 < argc) volume_fraction = std::atof(argv[++i]);
        else if (a == "--penal" && i + 1 < argc) penal = std::atoi(argv[++i]);
        else if (a == "--filter-passes" && i + 1 < argc) filter_passes = std::atoi(argv[++i]);
        else if (a == "--field-cg" && i + 1 < argc) field_cg = std::atoi(argv[++i]);
        else if (a == "--nodes" && i + 1 < argc) nodes_out = argv[++i];
        else if (a == "--elements" && i + 1 < argc) elements_out = argv[++i];
        else if (a == "--rel" && i + 1 < argc) rel = std::atof(argv[++i]);
        else if (input.empty()) input = a;
        else if (mesh.empty()) mesh = a;
        else die({MagnetiteError::Input, "Unrecognized argument " + a});
    }
    if (input.empty() || mesh.empty()) {
        std::fprintf(stderr, "usage: magnetite_gpu <input.json> <mesh.msh> [--nodes F] [--elements F] [--dry-run] [--rel TOL] [--stress-recovery] [--modal P --density RHO] [--transient STEPS --dt DT --density RHO [--rayleigh A,E] [--probe DOF]... [--kinematics linear|tl [--newton-tol T]]] [--explicit STEPS --density RHO [--dt DT | --dt-scale S] [--rayleigh A,E] [--probe DOF]... [--record-every K] [--kinematics linear|tl]] [--nonlinear INCREMENTS [--newton-tol T] [--line-search H] [--probe DOF]...] [--material svk|neo-hooke] [--adapt R [--refine-fraction T] [--refine-split 1|3]] [--topopt ITERS [--volume-fraction F] [--penal P] [--filter-passes K] [--field-cg 0..3]]\n");
        return 2;
    }
    if (modal_modes < 0 || (modal_modes > 0 && !(density > 0.0))) die({MagnetiteError::Input, "--modal P needs P >= 1 and --density RHO > 0"});
    if (buckling_modes < 0 || buckling_subspace < 0 || (buckling_subspace > 0 && buckling_modes < 1))
        die({MagnetiteError::Input, "--buckling P needs P >= 1, and --subspace Q goes with it"});
    if (transient && (transient_steps < 1 || !(dt > 0.0) || !(density > 0.0) || rayleigh_mass < 0.0 || rayleigh_stiffness < 0.0))
        die({MagnetiteError::Input, "--transient STEPS needs STEPS >= 1, --dt DT > 0, --density RHO > 0 and --rayleigh A,E >= 0"});
    if (explicit_run && (explicit_steps < 1 || dt < 0.0 || dt_scale < 0.0 || (dt > 0.0 && dt_scale > 0.0) || !(density > 0.0) || rayleigh_mass < 0.0 ||
                         rayleigh_stiffness < 0.0 || record_every < 1))
        die({MagnetiteError::Input, "--explicit STEPS needs STEPS >= 1, --density RHO > 0, --dt DT > 0 or --dt-scale S > 0 (not both), --rayleigh A,E >= 0 and --record-every K >= 1"});
    if (explicit_run && transient) die({MagnetiteError::Input, "--explicit and --transient share --dt, --rayleigh and --probe: one of them at a time"});
    if (!explicit_run && (dt_scale != 0.0 || record_every != 1)) die({MagnetiteError::Input, "--dt-scale and --record-every need --explicit STEPS"});
    if (!kinematics.empty() && !explicit_run && !transient) die({MagnetiteError::Input, "--kinematics needs --explicit STEPS or --transient STEPS"});
    if (!kinematics.empty() && kinematics != "linear" && kinematics != "tl")
        die({MagnetiteError::Input, "--kinematics " + kinematics + ": linear or tl (with --explicit STEPS or --transient STEPS)"});
    const bool total_lagrangian = kinematics == "tl";
    if (total_lagrangian && rayleigh_stiffness != 0.0)
        die({MagnetiteError::Input, std::string(transient ? "--transient" : "--explicit") +
                                        " with --kinematics tl takes --rayleigh A,0: stiffness-proportional damping is not objective"});
    const bool transient_tl = transient && total_lagrangian;
    const bool nonlinear_run = nonlinear != -1;
    if (nonlinear_run && (nonlinear < 1 || newton_tol < 0.0 || line_search < 0))
        die({MagnetiteError::Input, "--nonlinear INCREMENTS needs INCREMENTS >= 1, --newton-tol T >= 0 and --line-search H >= 0"});
    if (transient_tl && newton_tol < 0.0) die({MagnetiteError::Input, "--transient STEPS --kinematics tl needs --newton-tol T >= 0"});
    if (!nonlinear_run && ((newton_tol != 0.0 && !transient_tl) || line_search != 0))
        die({MagnetiteError::Input, "--newton-tol and --line-search need --nonlinear INCREMENTS (--newton-tol also goes with --transient STEPS --kinematics tl)"});
    if (nonlinear_run && (transient || explicit_run)) die({MagnetiteError::Input, "--nonlinear shares --probe with --transient and --explicit: one of them at a time"});
    if (!material.empty() && material != "svk" && material != "neo-hooke") die({MagnetiteError::Input, "--material " + material + ": svk or neo-hooke"});
    if (!material.empty() && !nonlinear_run && !total_lagrangian)
        die({MagnetiteError::Input, "--material needs --nonlinear INCREMENTS, or --explicit STEPS / --transient STEPS with --kinematics tl: the linear passes read no material law"});
    const bool neo_hooke = material == "neo-hooke";
    if (nonlinear_run && adapt > 0) die({MagnetiteError::Input, "--nonlinear solves on the mesh as given: not together with --adapt"});
    if (!transient && !explicit_run && (dt != 0.0 || (!probes.empty() && !nonlinear_run) || rayleigh_mass != 0.0 || rayleigh_stiffness != 0.0))
        die({MagnetiteError::Input, "--dt, --rayleigh and --probe need --transient STEPS"});
    if (adapt < 0 || !(refine_fraction > 0.0 && refine_fraction <= 1.0) || (refine_split != 1 && refine_split != 3))
        die({MagnetiteError::Input, "--adapt R needs R >= 0, --refine-fraction T in (0, 1] and --refine-split 1 or 3"});
    if (topopt < 0 || !(volume_fraction > 0.0 && volume_fraction <= 1.0) || penal < 1 || penal > 8 || filter_passes < 0 || filter_passes > 8)
        die({MagnetiteError::Input, "--topopt ITERS needs ITERS >= 0, --volume-fraction F in (0, 1], --penal 1..8 and --filter-passes 0..8"});
    if (field_cg < 0 || field_cg > 3 || (field_cg != 0 && topopt == 0))
        die({MagnetiteError::Input, "--field-cg K needs K in 0..3 (0 CSR phase, 1 plain, 2 Jacobi, 3 block-Jacobi on K's block rows) and --topopt"});
    if (explicit_run && adapt > 0) die({MagnetiteError::Input, "--explicit steps the mesh as given: not together with --adapt"});
    if (transient && adapt > 0) die({MagnetiteError::Input, "--transient steps the mesh as given: not together with --adapt"});
    if (topopt > 0 && adapt > 0) die({MagnetiteError::Input, "--topopt designs on the mesh as given: not together with --adapt"});
    // mesher::run (mesher.rs:939-974) minus geometry parsing and the gmsh subprocess
    const std::string text = slurp(input, MagnetiteError::Input, "Unable to open input file " + input);
    JsonParser jp(text);
    const Json doc = jp.value();
    // load_input_file's checks in its order, messages verbatim (mesher.rs:733-755; "in metadata section" for
    // boundary_conditions is the reference's own wording)
    if (!doc.has("metadata")) die({MagnetiteError::Input, "Input json missing metadata field"});
    if (!doc.has("boundary_conditions"))
        die({MagnetiteError::Input, "Input json missing boundary_conditions field in metadata section"});
    for (const char *k : {"part_thickness", "material_elasticity", "poisson_ratio"})
        if (!doc.get("metadata")->has(k))
            die({MagnetiteError::Input, std::string("Input json missing ") + k + " field in metadata section"});
    const ModelMetadata meta = parse_input_metadata(doc);
    std::vector<Node> nodes;
    std::vector<Element> elements;
    parse_mesh(mesh, nodes, elements);
    apply_boundary_conditions(parse_boundary_rules(doc), nodes);
    if (dry) {
        size_t ku = 0, kf = 0;
        double su = 0.0, sf = 0.0;
        for (const Node &n : nodes) {
            ku += n.ux.has_value() + n.uy.has_value();
            kf += n.fx.has_value() + n.fy.has_value();
            su += n.ux.value_or(0.0) + n.uy.value_or(0.0);
            sf += n.fx.value_or(0.0) + n.fy.value_or(0.0);
        }
        std::printf("dry-run: nodes %zu elements %zu prescribed_u %zu prescribed_f %zu sum_u %s sum_f %s E %s nu %s t %s first %zu,%zu,%zu\n",
                    nodes.size(), elements.size(), ku, kf, rust_display(su).c_str(), rust_display(sf).c_str(),
                    rust_display(meta.youngs_modulus).c_str(), rust_display(meta.poisson_ratio).c_str(),
                    rust_display(meta.part_thickness).c_str(), elements.empty() ? 0 : elements[0].nodes[0],
                    elements.empty() ? 0 : elements[0].nodes[1], elements.empty() ? 0 : elements[0].nodes[2]);
        if (transient)
            std::printf("dry-run: transient steps %d dt %s density %s rayleigh %s,%s probes %zu\n", transient_steps, rust_display(dt).c_str(),
                        rust_display(density).c_str(), rust_display(rayleigh_mass).c_str(), rust_display(rayleigh_stiffness).c_str(), probes.size());
        if (explicit_run)
            std::printf("dry-run: explicit steps %d dt %s dt_scale %s density %s rayleigh %s,%s probes %zu record_every %d\n", explicit_steps,
                        rust_display(dt).c_str(), rust_display(dt_scale).c_str(), rust_display(density).c_str(), rust_display(rayleigh_mass).c_str(),
                        rust_display(rayleigh_stiffness).c_str(), probes.size(), record_every);
        if (explicit_run && !kinematics.empty())
            std::printf("dry-run: explicit kinematics %s\n", total_lagrangian ? "total-lagrangian" : "linear");
        if (transient && !kinematics.empty())
            std::printf("dry-run: transient kinematics %s newton_tol %s\n", total_lagrangian ? "total-lagrangian" : "linear",
                        rust_display(newton_tol).c_str());
        if (!material.empty()) std::printf("dry-run: material %s\n", material.c_str());
        if (nonlinear_run)
            std::printf("dry-run: nonlinear increments %d newton_tol %s line_search %d probes %zu\n", nonlinear, rust_display(newton_tol).c_str(),
                        line_search, probes.size());
        return 0;
    }
    // solver::run (main.rs:64)
    mag_options opt;
    mag_default_options(&opt);
    opt.verbose = 1;
    if (rel > 0.0) {
        opt.stop_mode = MAG_STOP_REL;
        opt.tol = rel;
    }
    std::vector<Node> posed = recover || modal_modes > 0 || buckling_modes > 0 || topopt > 0 || transient || explicit_run || nonlinear_run ? nodes : std::vector<Node>();  // (run() fills every value in)
    if (adapt > 0) {
        RefineSpec spec;
        spec.theta = refine_fraction;
        spec.split = refine_split;
        std::vector<AdaptRound> history;
        if (Result err = solver::upload_refined(nodes, elements, meta, spec, adapt, history, &opt, &posed)) die(*err);
        for (size_t r = 0; r < history.size(); ++r)
            std::printf("info: adapt round %zu: %zu nodes, %zu elements, eta_rel %s\n", r, history[r].nodes, history[r].elements,
                        rust_display(history[r].eta_rel).c_str());
    } else if (Result err = solver::run(nodes, elements, meta, &opt)) {
        die(*err);
    }
    if (!material.empty()) { // (the law of the total-Lagrangian pass asked for below: solver::set_material_law)
        if (Result err = solver::set_material_law(neo_hooke ? MAG_LAW_NEO_HOOKE : MAG_LAW_SVK)) die(*err);
        std::printf("info: material %s\n", material.c_str());
    }
    if (nonlinear_run) {
        // The pass needs every element counter-clockwise, as the modal analysis does: the elements go in by their true sign.
        std::vector<Element> ccw = elements;
        for (Element &e : ccw)
            if (solver::compute_element_area(e, posed) < 0.0) std::swap(e.nodes[0], e.nodes[2]);
        opt.verbose = 0;
        NewtonSpec spec;
        spec.increments = nonlinear;
        spec.newton_tol = newton_tol;
        spec.line_search = line_search;
        spec.probes = probes;
        Newton nl;
        if (Result err = solver::run_newton(posed, ccw, meta, spec, nl, &opt)) die(*err);
        size_t at = 0;
        for (int k = 1; k <= nl.increments_converged; ++k) {
            int cg = 0;
            for (int i = 0; i < nl.newton_iterations[(size_t)k]; ++i) cg += nl.cg_iterations[at + (size_t)i];
            at += (size_t)nl.newton_iterations[(size_t)k];
            std::printf("info: increment %d load %s newton %d cg %d residual %s\n", k, rust_display(nl.load[(size_t)k]).c_str(),
                        (int)nl.newton_iterations[(size_t)k], cg, rust_display(nl.residuals[at - 1]).c_str());
        }
        if (!nl.converged) std::printf("warning: nonlinear: %s\n", nl.message.c_str());
        if (nl.inverted) std::printf("warning: nonlinear: an element was inverted (det F <= 0)\n");
        // nodes.csv / elements.csv carry the nonlinear result: u, and the von Mises value of the second Piola-Kirchhoff stress
        for (size_t i = 0; i < nodes.size(); ++i) nodes[i].ux = nl.u[2 * i], nodes[i].uy = nl.u[2 * i + 1];
        for (size_t e = 0; e < elements.size(); ++e) {
            const double sx = nl.elem[8 * e + 3], sy = nl.elem[8 * e + 4], sxy = nl.elem[8 * e + 5];
            elements[e].stress = std::sqrt(sx * sx - sx * sy + sy * sy + 3.0 * sxy * sxy);
        }
        load_path_output(nl, probes, load_path_name(nodes_out));
    }
    // post_processor::csv_output (main.rs:69); the matplotlib plot (main.rs:72) is not part of this tool
    csv_output(elements, nodes, nodes_out, elements_out);
    if (recover) {
        opt.verbose = 0;
        std::vector<StressField> fields;
        if (Result err = solver::stress_recovery(posed, elements, meta, {}, {}, fields, &opt)) die(*err);
        stress_output(fields[0], stress_name(nodes_out), stress_name(elements_out));
        std::printf("info: stress recovery eta_rel %s (eta %s, energy norm %s), largest von Mises stress %s in an element, %s at a node\n",
                    rust_display(fields[0].eta_rel).c_str(), rust_display(fields[0].eta).c_str(), rust_display(fields[0].energy_norm).c_str(),
                    rust_display(fields[0].vm_max).c_str(), rust_display(fields[0].vm_node_max).c_str());
    }
    if (modal_modes > 0) {
        // The modal analysis needs every element counter-clockwise (the stiffness carries the signed area).  check_ccw compares
        // the area with 1.0 (parse_mesh), which leaves a part of small elements clockwise: the elements go in by their true sign.
        std::vector<Element> ccw = elements;
        for (Element &e : ccw)
            if (solver::compute_element_area(e, posed) < 0.0) std::swap(e.nodes[0], e.nodes[2]);
        opt.verbose = 0;
        ModalSpec spec;
        spec.modes = modal_modes;
        spec.density = density;
        Modes modes;
        if (Result err = solver::modal(posed, ccw, meta, spec, modes, &opt)) die(*err);
        for (size_t k = 0; k < modes.lambda.size(); ++k)
            std::printf("info: mode %zu frequency %s Hz residual %s\n", k + 1, rust_display(modes.frequency[k]).c_str(),
                        rust_display(modes.residual[k]).c_str());
        modes_output(modes, posed.size(), modes_name(nodes_out));
    }
    if (buckling_modes > 0) {
        // The pass needs every element counter-clockwise, as the modal analysis does: the elements go in by their true sign.
        std::vector<Element> ccw = elements;
        for (Element &e : ccw)
            if (solver::compute_element_area(e, posed) < 0.0) std::swap(e.nodes[0], e.nodes[2]);
        opt.verbose = 0;
        BucklingSpec spec;
        spec.modes = buckling_modes;
        spec.subspace = buckling_subspace;
        BucklingModes bm;
        if (Result err = solver::buckling(posed, ccw, meta, spec, bm, &opt)) die(*err);
        for (size_t k = 0; k < bm.load_factor.size(); ++k)
            std::printf("info: buckling mode %zu load factor %s residual %s\n", k + 1, rust_display(bm.load_factor[k]).c_str(),
                        rust_display(bm.residual[k]).c_str());
        if (!bm.converged) std::printf("warning: buckling: stopped at the cap of outer steps above the tolerance\n");
        shapes_output(bm.shapes, bm.load_factor.size(), posed.size(), buckling_modes_name(nodes_out), "buckling shapes");
    }
    if (transient_tl) {
        // The pass needs every element counter-clockwise, as the modal analysis does: the elements go in by their true sign.
        std::vector<Element> ccw = elements;
        for (Element &e : ccw)
            if (solver::compute_element_area(e, posed) < 0.0) std::swap(e.nodes[0], e.nodes[2]);
        opt.verbose = 0;
        TransientTlSpec spec;
        spec.steps = transient_steps;
        spec.dt = dt;
        spec.density = density;
        spec.rayleigh_mass = rayleigh_mass;
        spec.newton_tol = newton_tol;
        spec.probes = probes;
        TransientTl tt;
        if (Result err = solver::transient_tl(posed, ccw, meta, spec, tt, &opt)) die(*err);
        std::printf("info: transient kinematics total-lagrangian\n");
        for (size_t n = 0; n < tt.run.iterations.size(); ++n)
            std::printf("info: step %zu t %s newton %d iterations %d\n", n, rust_display((double)n * dt).c_str(), (int)tt.newton_iterations[n],
                        (int)tt.run.iterations[n]);
        if (!tt.converged) std::printf("warning: transient: %s\n", tt.message.c_str());
        if (tt.inverted) std::printf("warning: transient: an element was inverted (det F <= 0)\n");
        history_output(tt.run, probes, dt, history_name(nodes_out));
    } else if (transient) {
        // The pass needs every element counter-clockwise, as the modal analysis does: the elements go in by their true sign.
        std::vector<Element> ccw = elements;
        for (Element &e : ccw)
            if (solver::compute_element_area(e, posed) < 0.0) std::swap(e.nodes[0], e.nodes[2]);
        opt.verbose = 0;
        TransientSpec spec;
        spec.steps = transient_steps;
        spec.dt = dt;
        spec.density = density;
        spec.rayleigh_mass = rayleigh_mass;
        spec.rayleigh_stiffness = rayleigh_stiffness;
        spec.probes = probes;
        Transient tr;
        if (Result err = solver::transient(posed, ccw, meta, spec, tr, &opt)) die(*err);
        for (size_t n = 0; n < tr.iterations.size(); ++n)
            std::printf("info: step %zu t %s iterations %d\n", n, rust_display((double)n * dt).c_str(), (int)tr.iterations[n]);
        history_output(tr, probes, dt, history_name(nodes_out));
    }
    if (explicit_run) {
        // The pass needs every element counter-clockwise, as the modal analysis does: the elements go in by their true sign.
        std::vector<Element> ccw = elements;
        for (Element &e : ccw)
            if (solver::compute_element_area(e, posed) < 0.0) std::swap(e.nodes[0], e.nodes[2]);
        opt.verbose = 0;
        ExplicitSpec spec;
        spec.steps = explicit_steps;
        spec.dt = dt;
        if (dt_scale > 0.0) spec.dt_scale = dt_scale;
        spec.density = density;
        spec.rayleigh_mass = rayleigh_mass;
        spec.rayleigh_stiffness = rayleigh_stiffness;
        spec.probes = probes;
        spec.record_every = record_every;
        spec.kinematics = total_lagrangian ? MAG_KIN_TOTAL_LAGRANGIAN : MAG_KIN_LINEAR;
        Explicit ex;
        if (Result err = solver::run_explicit(posed, ccw, meta, spec, ex, &opt)) die(*err);
        if (total_lagrangian) std::printf("info: explicit kinematics total-lagrangian\n");
        if (ex.inverted) std::printf("warning: explicit: an element was inverted (det F <= 0)\n");
        std::printf("info: explicit dt %s (bound %s)\n", rust_display(ex.dt).c_str(), rust_display(ex.dt_bound).c_str());
        std::vector<std::size_t> step;
        for (size_t n = 0; n < ex.time.size(); ++n) {
            step.push_back(n * (size_t)ex.record_every);
            std::printf("info: step %zu t %s\n", step[n], rust_display(ex.time[n]).c_str());
        }
        history_output(ex.time, step, ex.probe_u, ex.probe_v, ex.probe_a, probes, history_name(nodes_out));
    }
    if (topopt > 0) {
        // The density design needs every element counter-clockwise, as the modal analysis does: the elements go in by their true sign.
        std::vector<Element> ccw = elements;
        for (Element &e : ccw)
            if (solver::compute_element_area(e, posed) < 0.0) std::swap(e.nodes[0], e.nodes[2]);
        opt.verbose = 0;
        opt.field_cg = field_cg; // (the CG of every design iteration: mag_options.field_cg)
        DesignSpec spec;
        spec.volume_fraction = volume_fraction;
        spec.penal = penal;
        spec.filter_passes = filter_passes;
        FieldSession session;
        if (Result err = solver::design_init(session, posed, ccw, meta, spec, &opt)) die(*err);
        for (int k = 0; k < topopt; ++k) {
            DesignInfo info;
            if (Result err = solver::design_step(session, &info)) die(*err);
            std::printf("info: topopt iteration %d: J %s, volume %s, change %s\n", k, rust_display(info.J).c_str(),
                        rust_display(info.volume_fraction).c_str(), rust_display(info.change).c_str());
        }
        Design design;
        if (Result err = solver::download_design(session, design)) die(*err);
        density_output(design, density_name(elements_out));
    }
    return 0;
}
