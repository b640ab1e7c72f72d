// Host-only check of sym_pencil_eig (csrc/modal_host.h, the Rayleigh-Ritz step of mag_run_buckling): pencils B q = mu A q built
// from known mu of both signs -- A = M^T M and B = M^T diag(mu) M with a seeded, well-conditioned M -- for n = 1, 2, 14 and 32,
// among the mu a zero and a +- pair of equal magnitude; it prints n, A, B, the mu it was built from ("exact"), the mu found and Q
// in hex (tests/test_buckling_cpp.py does the arithmetic), then a rank-deficient A, which must be refused with its column
// named.  Built by g++ alone, with the address and undefined-behaviour sanitizers where they link.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "modal_host.h"

namespace {

uint64_t g_state = 0x2545f4914f6cdd1dull;
double uniform() // splitmix64, in (-1, 1)
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) / 4503599627370496.0 - 1.0;
}

// I + 0.3 U / sqrt(n), U uniform in (-1, 1): nonsingular, of condition below 4
std::vector<double> mixing(int n)
{
    std::vector<double> m((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) m[(size_t)i * n + j] = (i == j ? 1.0 : 0.0) + 0.3 * uniform() / std::sqrt((double)n);
    return m;
}

// M^T diag(d) M
std::vector<double> congruence(int n, const std::vector<double> &m, const std::vector<double> &d)
{
    std::vector<double> out((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += m[(size_t)k * n + i] * d[(size_t)k] * m[(size_t)k * n + j];
            out[(size_t)i * n + j] = out[(size_t)j * n + i] = s;
        }
    return out;
}

void print(const char *name, const std::vector<double> &v)
{
    printf("%s", name);
    for (double x : v) printf(" %a", x);
    printf("\n");
}

int solve_and_print(int n, const std::vector<double> &A, const std::vector<double> &B, const std::vector<double> &exact)
{
    std::vector<double> mu((size_t)n), Q((size_t)n * n);
    int pivot = -1;
    double least = -1.0;
    const int rc = magh::sym_pencil_eig(n, A.data(), B.data(), mu.data(), Q.data(), &pivot, &least);
    printf("pair %d status %d pivot %d\n", n, rc, pivot);
    print("A", A);
    print("B", B);
    print("exact", exact);
    print("least", {least});
    if (rc == magh::EIG_OK) {
        print("mu", mu);
        print("Q", Q);
    }
    return rc;
}

} // namespace

int main()
{
    const std::vector<std::vector<double>> known = {
        {-0.75},
        {0.5, -0.5},
        {1.0, -0.875, 0.75, 0.5, -0.5, 0.4375, -0.3125, 0.25, 0.125, -0.0625, 0.03125, -1e-3, 1e-6, 0.0},
        {1.0,    -0.96875, 0.9375, 0.875, -0.875, 0.8125, -0.75,  0.6875, 0.625, -0.5625, 0.5,  -0.4375, 0.375, 0.3125, -0.25, 0.1875,
         0.125, -0.0625,   0.03125, -0.015625, 1e-2, -1e-3, 1e-4, -1e-5, 1e-6, -1e-7, 1e-8, -1e-9, 1e-10, -1e-12, 0.0, 0.0},
    };
    for (const std::vector<double> &mu : known) {
        const int n = (int)mu.size();
        const std::vector<double> m = mixing(n);
        if (solve_and_print(n, congruence(n, m, std::vector<double>((size_t)n, 1.0)), congruence(n, m, mu), mu) != magh::EIG_OK) return 1;
    }
    { // a rank-deficient A: its third vector is the sum of the first two (the pivot refusal), B of both signs
        const int n = 3;
        const double v[3][3] = {{1.0, 2.0, 0.5}, {0.0, 1.0, -1.0}, {1.0, 3.0, -0.5}};
        std::vector<double> A(9, 0.0), B = {1.0, 0.0, 0.0, 0.0, -2.0, 0.0, 0.0, 0.0, 0.5};
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                for (int k = 0; k < 3; ++k) A[(size_t)i * n + j] += v[i][k] * v[j][k];
        if (solve_and_print(n, A, B, {0.0, 0.0, 0.0}) != magh::EIG_DEPENDENT) return 1;
    }
    { // an A whose diagonal is not positive: refused with that column, nothing factored
        const std::vector<double> A = {1.0, 0.0, 0.0, 0.0}, B = {1.0, 0.0, 0.0, -1.0};
        if (solve_and_print(2, A, B, {0.0, 0.0}) != magh::EIG_DEPENDENT) return 1;
    }
    // bad arguments
    double one = 1.0, out = 0.0, q = 0.0;
    if (magh::sym_pencil_eig(0, &one, &one, &out, &q, nullptr) != magh::EIG_BAD_ARGS) return 1;
    if (magh::sym_pencil_eig(33, &one, &one, &out, &q, nullptr) != magh::EIG_BAD_ARGS) return 1;
    if (magh::sym_pencil_eig(1, nullptr, &one, &out, &q, nullptr) != magh::EIG_BAD_ARGS) return 1;
    return 0;
}
