// Internal, host only (no HIP include: a host compiler alone builds it; tests/cpp/modal_eig.cpp and pencil_eig.cpp do): the
// Rayleigh-Ritz steps of mag_run_modal and (sym_pencil_eig, at the end) of mag_run_buckling.  The former -- the generalised eigenproblem A q = lambda B q of two symmetric positive definite matrices for n <= 32.
//   A and B scaled to A's unit diagonal (S = diag(A)^-1/2: A_s = S A S, B_s = S B S),  A_s = L L^T (Cholesky),
//   C = L^-1 B_s L^-T,  C = V diag(mu) V^T by cyclic Jacobi to convergence,  lambda = 1 / mu,  Q = S L^-T V diag(mu)^-1/2,
// the pairs sorted ascending in lambda (equal values in the order Jacobi left them), so that Q^T B Q = I and
// Q^T A Q = diag(lambda), and every column of Q with its entry of largest magnitude positive (the first on a tie): the same
// input gives the same bits.
// Why A is the matrix factored: with Z = K^-1 Y, A = Z^T K Z carries the spread lambda_q / lambda_1 of the subspace where
// B = Z^T M Z carries its square -- at the first outer step, where the columns of Z are no Ritz vectors yet, a slender part's B
// has a condition beyond 1e13 and no Cholesky of it is to be trusted, while A's stays at its square root.  The large mu
// (the lowest modes) come out of Jacobi to round-off; a small mu (a guard vector) to round-off of the largest.
// What is refused (EIG_DEPENDENT): a Cholesky pivot of A_s at or below kEigPivotTol (each pivot stands against its own column:
// the diagonal is 1), and a mu at or below kEigPivotTol times the largest (B deficient where A is not).
#pragma once
#include <cmath>

namespace magh {

constexpr int kEigMaxN = 32;
constexpr double kEigPivotTol = 1e-13; // a pivot of the unit-diagonal A, or mu_min / mu_max, at or below this: dependent vectors

enum { EIG_OK = 0, EIG_BAD_ARGS = 1, EIG_DEPENDENT = 2, EIG_NO_CONVERGENCE = 3 };

// the column with the smallest Cholesky pivot of the n x n matrix M (row major, the lower triangle is read) scaled to a unit
// diagonal, a pivot that is not positive ending the search: names the dependent column where EIG_DEPENDENT comes from B
inline int weakest_column(int n, const double *M)
{
    constexpr int S = kEigMaxN;
    double L[S][S] = {}, d[S];
    for (int i = 0; i < n; ++i) {
        if (!(M[i * n + i] > 0.0)) return i;
        d[i] = 1.0 / std::sqrt(M[i * n + i]);
    }
    int at = 0;
    double least = 2.0;
    for (int j = 0; j < n; ++j) {
        double s = 1.0;
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (s < least) {
            least = s;
            at = j;
        }
        if (!(s > 0.0)) return j;
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < n; ++i) {
            double t = d[i] * M[i * n + j] * d[j];
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    return at;
}

// ---- what the two Ritz functions below share: the work arrays and the steps on them, each step the same operations in the same
// order for both
struct EigWork {
    double L[kEigMaxN][kEigMaxN] = {}, C[kEigMaxN][kEigMaxN] = {}, V[kEigMaxN][kEigMaxN] = {}, d[kEigMaxN];
};

// d = diag(A)^-1/2 and A_s = L L^T.  False with (*column, *figure) where a diagonal entry or a pivot is refused; *low: the
// smallest pivot
inline bool eig_factor(int n, const double *A, EigWork &w, double *low, int *column, double *figure)
{
    for (int i = 0; i < n; ++i) {
        const double a = A[i * n + i];
        if (!(a > 0.0) || !std::isfinite(a)) {
            *column = i, *figure = a;
            return false;
        }
        w.d[i] = 1.0 / std::sqrt(a);
    }
    for (int j = 0; j < n; ++j) {
        double s = 1.0;
        for (int k = 0; k < j; ++k) s -= w.L[j][k] * w.L[j][k];
        if (!(s > kEigPivotTol) || !std::isfinite(s)) {
            *column = j, *figure = s;
            return false;
        }
        *low = std::fmin(*low, s);
        w.L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < n; ++i) {
            double t = w.d[i] * A[i * n + j] * w.d[j];
            for (int k = 0; k < j; ++k) t -= w.L[i][k] * w.L[j][k];
            w.L[i][j] = t / w.L[j][j];
        }
    }
    return true;
}

// C = L^-1 B_s L^-T: T = L^-1 B_s column by column, then C^T = L^-1 T^T row by row; the mean of both triangles.  V = I
inline void eig_reduce(int n, const double *B, EigWork &w)
{
    for (int c = 0; c < n; ++c)
        for (int i = 0; i < n; ++i) {
            double t = w.d[i] * (i >= c ? B[i * n + c] : B[c * n + i]) * w.d[c];
            for (int k = 0; k < i; ++k) t -= w.L[i][k] * w.C[k][c];
            w.C[i][c] = t / w.L[i][i];
        }
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < n; ++i) {
            double t = w.C[r][i];
            for (int k = 0; k < i; ++k) t -= w.L[i][k] * w.V[r][k];
            w.V[r][i] = t / w.L[i][i];
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) w.C[i][j] = w.C[j][i] = 0.5 * (w.V[i][j] + w.V[j][i]);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) w.V[i][j] = i == j ? 1.0 : 0.0;
}

// cyclic Jacobi on C (V: the rotations' product): sweeps over (p, q), p < q, until every off-diagonal entry is zero or negligible
// against both of its diagonal entries.  False: no convergence in 64 sweeps
inline bool eig_jacobi(int n, EigWork &w)
{
    auto &C = w.C;
    auto &V = w.V;
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
    return done;
}

// column k of Q = S L^-T V[:, src] scale, its entry of largest magnitude positive (the first on a tie)
inline void eig_column(int n, const EigWork &w, int src, double scale, double *Q, int k)
{
    double col[kEigMaxN];
    for (int i = n - 1; i >= 0; --i) {
        double t = w.V[i][src];
        for (int m = i + 1; m < n; ++m) t -= w.L[m][i] * col[m];
        col[i] = t / w.L[i][i];
    }
    for (int i = 0; i < n; ++i) col[i] = w.d[i] * col[i] * scale;
    int big = 0;
    for (int i = 1; i < n; ++i)
        if (std::fabs(col[i]) > std::fabs(col[big])) big = i;
    const double sign = col[big] < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < n; ++i) Q[i * n + k] = sign * col[i];
}

// A, B: n x n row major, symmetric (the lower triangles are read), positive definite.  lambda: n.  Q: n x n row major, column k
// = vector k.  *pivot: with EIG_DEPENDENT, the column whose pivot failed.  *least (may be null): the smallest figure that was
// tested against kEigPivotTol (on EIG_DEPENDENT the failing one).
inline int sym_def_eig(int n, const double *A, const double *B, double *lambda, double *Q, int *pivot, double *least = nullptr)
{
    if (n < 1 || n > kEigMaxN || !A || !B || !lambda || !Q) return EIG_BAD_ARGS;
    EigWork w;
    double low = 1.0;
    const auto dependent = [&](int column, double figure) {
        if (pivot) *pivot = column;
        if (least) *least = figure;
        return (int)EIG_DEPENDENT;
    };
    int column = 0;
    double figure = 0.0;
    if (!eig_factor(n, A, w, &low, &column, &figure)) return dependent(column, figure);
    eig_reduce(n, B, w);
    if (!eig_jacobi(n, w)) return EIG_NO_CONVERGENCE;
    // ---- mu descending = lambda ascending (insertion sort: stable), Q = S L^-T V diag(mu)^-1/2, signs
    int order[kEigMaxN];
    for (int k = 0; k < n; ++k) {
        int at = k;
        while (at > 0 && w.C[order[at - 1]][order[at - 1]] < w.C[k][k]) {
            order[at] = order[at - 1];
            --at;
        }
        order[at] = k;
    }
    const double mu_top = w.C[order[0]][order[0]], mu_low = w.C[order[n - 1]][order[n - 1]];
    if (!(mu_low > kEigPivotTol * mu_top) || !std::isfinite(mu_top)) return dependent(weakest_column(n, B), mu_low / mu_top);
    low = std::fmin(low, mu_low / mu_top);
    if (least) *least = low;
    for (int k = 0; k < n; ++k) {
        const double mu = w.C[order[k]][order[k]];
        lambda[k] = 1.0 / mu;
        eig_column(n, w, order[k], 1.0 / std::sqrt(mu), Q, k);
    }
    return EIG_OK;
}

// The Ritz step of mag_run_buckling: the pencil B q = mu A q with A symmetric positive definite and B symmetric of ANY signature
// (B = -Z^T K_G Z is indefinite), for n <= 32.  A is scaled to a unit diagonal and factored as above (the same pivot rule), C =
// L^-1 B_s L^-T is diagonalised by the same Jacobi; the pairs are ordered by |mu| descending (equal magnitudes in the order
// Jacobi left them) and Q = S L^-T V, so that Q^T A Q = I and Q^T B Q = diag(mu); the column signs are sym_def_eig's.  B may be
// singular: a mu may be zero.  EIG_DEPENDENT (with *pivot, *least as above) comes from A alone.
inline int sym_pencil_eig(int n, const double *A, const double *B, double *mu, double *Q, int *pivot, double *least = nullptr)
{
    if (n < 1 || n > kEigMaxN || !A || !B || !mu || !Q) return EIG_BAD_ARGS;
    EigWork w;
    double low = 1.0;
    int column = 0;
    double figure = 0.0;
    if (!eig_factor(n, A, w, &low, &column, &figure)) {
        if (pivot) *pivot = column;
        if (least) *least = figure;
        return EIG_DEPENDENT;
    }
    eig_reduce(n, B, w);
    if (!eig_jacobi(n, w)) return EIG_NO_CONVERGENCE;
    int order[kEigMaxN];
    for (int k = 0; k < n; ++k) { // (insertion sort: stable)
        int at = k;
        while (at > 0 && std::fabs(w.C[order[at - 1]][order[at - 1]]) < std::fabs(w.C[k][k])) {
            order[at] = order[at - 1];
            --at;
        }
        order[at] = k;
    }
    if (!std::isfinite(w.C[order[0]][order[0]])) return EIG_NO_CONVERGENCE;
    if (least) *least = low;
    for (int k = 0; k < n; ++k) {
        mu[k] = w.C[order[k]][order[k]];
        eig_column(n, w, order[k], 1.0, Q, k);
    }
    return EIG_OK;
}

} // namespace magh
