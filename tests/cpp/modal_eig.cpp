// Host-only check of csrc/modal_host.h (the Rayleigh-Ritz step of mag_run_modal): for seeded symmetric positive definite pairs
// (A, B) it prints n, A, B, the eigenvalues and Q in hex (tests/test_modal.py does the arithmetic), then a rank-deficient B,
// which must be reported and not factored, then graded pairs as the first outer step of a slender part hands them over:
// A = G^T D G and B = G^T D^2 G with G orthogonal and B of condition 1e10 and 1e12, n = 12 and 32, their eigenvalues 1 / D
// printed as "exact".  Built by g++ alone, with the address and undefined-behaviour sanitizers where they link.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "modal_host.h"

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double uniform() // splitmix64, in (-1, 1)
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) / 4503599627370496.0 - 1.0;
}

// G^T G + shift I of a random n x n G
std::vector<double> spd(int n, double shift)
{
    std::vector<double> g((size_t)n * n), m((size_t)n * n, 0.0);
    for (double &v : g) v = uniform();
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = i == j ? shift : 0.0;
            for (int k = 0; k < n; ++k) s += g[(size_t)k * n + i] * g[(size_t)k * n + j];
            m[(size_t)i * n + j] = s;
        }
    return m;
}

// an orthogonal n x n G: the rows of a random matrix by Gram-Schmidt, twice
std::vector<double> orthogonal(int n)
{
    std::vector<double> g((size_t)n * n);
    for (double &v : g) v = uniform();
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < n; ++i) {
            double *gi = &g[(size_t)i * n];
            for (int k = 0; k < i; ++k) {
                const double *gk = &g[(size_t)k * n];
                double dot = 0.0;
                for (int c = 0; c < n; ++c) dot += gi[c] * gk[c];
                for (int c = 0; c < n; ++c) gi[c] -= dot * gk[c];
            }
            double norm = 0.0;
            for (int c = 0; c < n; ++c) norm += gi[c] * gi[c];
            norm = std::sqrt(norm);
            for (int c = 0; c < n; ++c) gi[c] /= norm;
        }
    return g;
}

// G^T diag(d) G
std::vector<double> congruence(int n, const std::vector<double> &g, const std::vector<double> &d)
{
    std::vector<double> m((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < n; ++k) m[(size_t)i * n + j] += g[(size_t)k * n + i] * d[(size_t)k] * g[(size_t)k * n + j];
    return m;
}

void print(const char *name, const std::vector<double> &v)
{
    printf("%s", name);
    for (double x : v) printf(" %a", x);
    printf("\n");
}

int solve_and_print(int n, const std::vector<double> &A, const std::vector<double> &B)
{
    std::vector<double> lambda((size_t)n), Q((size_t)n * n);
    int pivot = -1;
    const int rc = magh::sym_def_eig(n, A.data(), B.data(), lambda.data(), Q.data(), &pivot);
    printf("pair %d status %d pivot %d\n", n, rc, pivot);
    print("A", A);
    print("B", B);
    if (rc == magh::EIG_OK) {
        print("lambda", lambda);
        print("Q", Q);
    }
    return rc;
}

} // namespace

int main()
{
    for (int n : {1, 2, 7, 12, 32}) {
        const std::vector<double> A = spd(n, 0.5), B = spd(n, 1.0);
        if (solve_and_print(n, A, B) != magh::EIG_OK) return 1;
    }
    { // two equal eigenvalues: A = 3 B on a 2-dimensional invariant subspace -- A = B D with D = diag(3, 3, 5, 7) in B's own
      // eigenbasis is not symmetric in general, so take B = I scaled and A diagonal with a repeated entry, rotated together
        const int n = 4;
        const double c = 0.8, s = 0.6, d[4] = {3.0, 7.0, 3.0, 5.0}, b[4] = {2.0, 1.0, 2.0, 0.5};
        // R = a rotation in the (0, 1) plane; A = R^T diag(d * b) R, B = R^T diag(b) R: the pairs are d
        double R[4][4] = {{c, s, 0, 0}, {-s, c, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
        std::vector<double> A(16, 0.0), B(16, 0.0);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                for (int k = 0; k < n; ++k) {
                    A[(size_t)i * n + j] += R[k][i] * d[k] * b[k] * R[k][j];
                    B[(size_t)i * n + j] += R[k][i] * b[k] * R[k][j];
                }
        if (solve_and_print(n, A, B) != magh::EIG_OK) return 1;
    }
    { // a rank-deficient B: its third vector is the sum of the first two
        const int n = 3;
        const double v[3][3] = {{1.0, 2.0, 0.5}, {0.0, 1.0, -1.0}, {1.0, 3.0, -0.5}};
        std::vector<double> A = spd(n, 0.5), B(9, 0.0);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                for (int k = 0; k < 3; ++k) B[(size_t)i * n + j] += v[i][k] * v[j][k];
        if (solve_and_print(n, A, B) != magh::EIG_DEPENDENT) return 1;
    }
    for (double cond : {1e10, 1e12})
        for (int n : {12, 32}) { // graded: D_k^2 from 1 down to 1 / cond, every column of G in every entry
            const std::vector<double> g = orthogonal(n);
            std::vector<double> d((size_t)n), d2((size_t)n), exact((size_t)n);
            for (int k = 0; k < n; ++k) {
                d[(size_t)k] = std::pow(cond, -0.5 * k / (n - 1));
                d2[(size_t)k] = d[(size_t)k] * d[(size_t)k];
                exact[(size_t)k] = 1.0 / d[(size_t)k];
            }
            if (solve_and_print(n, congruence(n, g, d), congruence(n, g, d2)) != magh::EIG_OK) return 1;
            print("exact", exact);
        }
    return 0;
}
