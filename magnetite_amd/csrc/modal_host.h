// Internal, host only (no HIP include: a host compiler alone builds it; tests/cpp/modal_eig.cpp does): the Rayleigh-Ritz step of
// mag_run_modal -- the symmetric-definite generalised eigenproblem A q = lambda B q for n <= 32.
//   B = L L^T (Cholesky),  C = L^-1 A L^-T,  C = V diag(lambda) V^T by cyclic Jacobi to convergence,  Q = L^-T V,
// the pairs sorted ascending (equal values in the order Jacobi left them), so that Q^T B Q = I and Q^T A Q = diag(lambda), and
// every column of Q with its entry of largest magnitude positive (the first on a tie): the same input gives the same bits.
#pragma once
#include <cmath>

namespace magh {

constexpr int kEigMaxN = 32;
constexpr double kEigPivotTol = 1e-13; // a Cholesky pivot <= this times the largest diagonal entry of B: dependent vectors

enum { EIG_OK = 0, EIG_BAD_ARGS = 1, EIG_DEPENDENT = 2, EIG_NO_CONVERGENCE = 3 };

// A, B: n x n row major, symmetric (the lower triangles are read).  lambda: n.  Q: n x n row major, column k = vector k.
// *pivot: with EIG_DEPENDENT, the column whose pivot failed.
inline int sym_def_eig(int n, const double *A, const double *B, double *lambda, double *Q, int *pivot)
{
    if (n < 1 || n > kEigMaxN || !A || !B || !lambda || !Q) return EIG_BAD_ARGS;
    constexpr int S = kEigMaxN;
    double L[S][S] = {}, C[S][S] = {}, V[S][S] = {};
    double top = 0.0;
    for (int i = 0; i < n; ++i) top = std::fmax(top, B[i * n + i]);
    // ---- B = L L^T
    for (int j = 0; j < n; ++j) {
        double s = B[j * n + j];
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > kEigPivotTol * top) || !std::isfinite(s)) {
            if (pivot) *pivot = j;
            return EIG_DEPENDENT;
        }
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < n; ++i) {
            double t = B[i * n + j];
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    // ---- C = L^-1 A L^-T: T = L^-1 A column by column, then C^T = L^-1 T^T row by row; the mean of both triangles
    for (int c = 0; c < n; ++c)
        for (int i = 0; i < n; ++i) {
            double t = i >= c ? A[i * n + c] : A[c * n + i];
            for (int k = 0; k < i; ++k) t -= L[i][k] * C[k][c];
            C[i][c] = t / L[i][i];
        }
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < n; ++i) {
            double t = C[r][i];
            for (int k = 0; k < i; ++k) t -= L[i][k] * V[r][k];
            V[r][i] = t / L[i][i];
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) C[i][j] = C[j][i] = 0.5 * (V[i][j] + V[j][i]);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    // ---- cyclic Jacobi: sweeps over (p, q), p < q, until every off-diagonal entry is zero or negligible against both of its
    // diagonal entries
    bool done = n == 1;
    for (int sweep = 0; sweep < 64 && !done; ++sweep) {
        done = true;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = C[p][q];
                if (apq == 0.0) continue;
                const double g = 100.0 * std::fabs(apq);
                if (std::fabs(C[p][p]) + g == std::fabs(C[p][p]) && std::fabs(C[q][q]) + g == std::fabs(C[q][q])) {
                    C[p][q] = C[q][p] = 0.0;
                    continue;
                }
                done = false;
                const double h = C[q][q] - C[p][p];
                double t;
                if (std::fabs(h) + g == std::fabs(h)) {
                    t = apq / h;
                } else {
                    const double theta = 0.5 * h / apq;
                    t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) { // columns p, q
                    const double kp = C[k][p], kq = C[k][q];
                    C[k][p] = c * kp - s * kq;
                    C[k][q] = s * kp + c * kq;
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - s * vq;
                    V[k][q] = s * vp + c * vq;
                }
                for (int k = 0; k < n; ++k) { // rows p, q
                    const double pk = C[p][k], qk = C[q][k];
                    C[p][k] = c * pk - s * qk;
                    C[q][k] = s * pk + c * qk;
                }
                C[p][q] = C[q][p] = 0.0;
            }
    }
    if (!done) return EIG_NO_CONVERGENCE;
    // ---- ascending (insertion sort: stable), Q = L^-T V, signs
    int order[S];
    for (int k = 0; k < n; ++k) {
        int at = k;
        while (at > 0 && C[order[at - 1]][order[at - 1]] > C[k][k]) {
            order[at] = order[at - 1];
            --at;
        }
        order[at] = k;
    }
    for (int k = 0; k < n; ++k) {
        const int src = order[k];
        lambda[k] = C[src][src];
        double col[S];
        for (int i = n - 1; i >= 0; --i) {
            double t = V[i][src];
            for (int m = i + 1; m < n; ++m) t -= L[m][i] * col[m];
            col[i] = t / L[i][i];
        }
        int big = 0;
        for (int i = 1; i < n; ++i)
            if (std::fabs(col[i]) > std::fabs(col[big])) big = i;
        const double sign = col[big] < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < n; ++i) Q[i * n + k] = sign * col[i];
    }
    return EIG_OK;
}

} // namespace magh
