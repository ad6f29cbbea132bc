// EPnP of PnPsolver (reference src/PnPsolver.cc:375-950: compute_pose and everything it calls) and CheckInliers (:308-339) for one correspondence.
// ONE source for the host (libsind_host.so: sindh_pnp_pose, sindh_pnp_check) and the device (../match_pnp.hip: k_pnp_pose, k_pnp_check), as peac_fit.hpp is:
// IEEE FP64 add / mul / div / sqrt on both sides and no contraction (-ffp-contract=off), so the two give the same bits.  Every sum is in the reference's order.
// No libm / ocml call besides sqrt and fabs: hypot is DEFINED here (epnp_hypot, the scaled-sqrt form OpenCV's lapack.cpp has and host/sim3.cpp:22 records).
//
// PARITY WITH A REAL OPENCV BUILD IS UNPINNED.  The reference calls OpenCV's C API; OpenCV is not available to build or run, so each primitive is restated
// from OpenCV 4.2.0 as remembered.  It matters most here: for a 4-point sample MtM (12 x 12) has rank <= 8, and compute_L_6x10 / compute_ccs read the four
// rows of U^T of the SMALLEST singular values.  Those rows are an arbitrary basis of a null space, so the hypothesis depends on the SVD down to its last bit
// and on its iteration order; an OpenCV built with LAPACK (HAVE_LAPACK routes SVD::compute to dgesdd) gives another basis and another hypothesis.
// tests/pnp_ref.py is the same restatement in Python (bit equality BY CONSTRUCTION); tests/test_pnp_cpu.py also recovers ground-truth poses, which shares
// none of the guesses.  [R] = recalled with confidence, [G] = guessed / uncertain.
//   cvMulTransposed(A, D, 1)            D = A^T A; below 100 rows / columns not gemm but MulTransposedR<double, double>: for i, for j >= i:
//                                       s = 0; s += A[k][i] * A[k][j], k ascending; D[i][j] = s * scale (1.0); then completeSymm copies the upper
//                                       triangle down, so D is symmetric to the bit                                                                  [R: the sum; G: the 100]
//                                       (the products with fill_M's literal zeros are formed and added: 0 * inf is a NaN there and here)
//   cvSVD(A, W, U, V, flags)            cv::SVD::compute: m >= n here, so At = A^T ([n][m], its rows are A's columns), JacobiSVD(At, W, Vt, m, n, n1 = n),
//                                       U^T = At afterwards, V^T = Vt.  SVD::operator() computes Vt even where the caller passes no V; it does not
//                                       influence At, so it is skipped for the 12 x 12 (wantV = false), but the zero-singular-value tail, which
//                                       the reference enters only with Vt != 0, still runs                                                           [R]
//                                       CV_SVD_U_T: the caller's U holds At (rows = left singular vectors); without it U = At^T; V = Vt^T            [R]
//   JacobiSVDImpl_<double>              one-sided Jacobi on the rows of At: W[i] = sum of squares of row i; max_iter = max(m, 30) sweeps over i < j;
//                                       p = sum Ai[k] * Aj[k]; skip if |p| <= eps * sqrt(a * b), eps = 10 DBL_EPSILON; p *= 2; beta = a - b;
//                                       gamma = hypot(p, beta); beta < 0: delta = (gamma - beta) * 0.5, s = sqrt(delta / gamma), c = p / (gamma * s * 2);
//                                       else c = sqrt((gamma + beta) / (gamma * 2)), s = p / (gamma * c * 2); t0 = c * Ai[k] + s * Aj[k],
//                                       t1 = -s * Ai[k] + c * Aj[k]; W[i], W[j] recomputed from the new rows; the same rotation on Vt; stop after a sweep
//                                       without rotation.  Then W[i] = sqrt(sum of squares), a selection sort descending that swaps rows of At and Vt,
//                                       and rows are scaled by 1 / W[i]                                                                               [R: all of it;
//                                       G: that VBLAS<double>::givens (SSE2, two lanes, mul and add) rounds as the scalar loop does]
//   the zero-singular-value tail        for i < n1 with W[i] <= DBL_MIN, up to 100 times: row i = +-1 / m by bit 8 of RNG(0x12345678).next()
//                                       (state = (unsigned)state * 4164903690 + (state >> 32), one generator per SVD call), two rounds of: for j < i
//                                       subtract the projection on row j, divide by the sum of magnitudes (0 if that is <= 100 eps); sd = the norm           [G: recalled in
//                                       outline, every detail uncertain; it runs only for an exactly zero row]
//   cvInvert(A, X, CV_SVD)              SVD::compute (no flags) and SVD::backSubst without a right side: SVBkSb with nb = m: threshold = 2 DBL_EPSILON *
//                                       sum W; X = 0; for i with |W[i]| > threshold: buffer[j] = U[j][i] * (1 / W[i]); X[r][j] = X[r][j] + Vt[i][r] * buffer[j]   [R]
//   cvSolve(A, b, x, CV_SVD)            6 x nc, nc < 6: At = A^T, JacobiSVD(At, W, Vt, 6, nc), SVBkSb with nb = 1: the same threshold; x = 0; for i:
//                                       s = sum_j At[i][j] * b[j]; s *= 1 / W[i]; x[j] = x[j] + s * Vt[i][j]                                         [R]
//   qr_solve on a singular A            returns with X untouched: in the reference X is then an uninitialised stack array in the first Gauss-Newton step.
//                                       DEFINED here: X starts as zeros                                                                              [G by necessity]
#pragma once
#include <cmath>
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include "peac_fit.hpp"                                              // SIND_HD

namespace sind {

SIND_HD inline double epnp_hypot(double a, double b) {
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
}

// JacobiSVDImpl_<double>(At, W, Vt, m, n, n1) with minval = DBL_MIN, eps = 10 DBL_EPSILON; At [n][m] and Vt [n][n] dense, n <= 12.  wantV = false leaves Vt alone (may be null).
SIND_HD inline void epnp_jacobi_svd(double* At, double* Wout, double* Vt, bool wantV, int m, int n, int n1) {
    const double eps = DBL_EPSILON * 10, minval = DBL_MIN;
    double W[12];
    int i, j, k, iter; const int max_iter = m > 30 ? m : 30;
    double c, s, sd;
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sd;
        if (wantV) { for (k = 0; k < n; k++) Vt[i * n + k] = 0; Vt[i * n + i] = 1; }
    }
    for (iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (i = 0; i < n - 1; i++) for (j = i + 1; j < n; j++) {
            double* Ai = At + i * m; double* Aj = At + j * m;
            double a = W[i], p = 0, b = W[j];
            for (k = 0; k < m; k++) p += Ai[k] * Aj[k];
            if (fabs(p) <= eps * sqrt(a * b)) continue;
            p *= 2;
            const double beta = a - b, gamma = epnp_hypot(p, beta);
            if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = sqrt(delta / gamma); c = p / (gamma * s * 2); }
            else { c = sqrt((gamma + beta) / (gamma * 2)); s = p / (gamma * c * 2); }
            a = b = 0;
            for (k = 0; k < m; k++) {
                const double t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
                Ai[k] = t0; Aj[k] = t1;
                a += t0 * t0; b += t1 * t1;
            }
            W[i] = a; W[j] = b;
            changed = true;
            if (wantV) {
                double* Vi = Vt + i * n; double* Vj = Vt + j * n;
                for (k = 0; k < n; k++) { const double t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k]; Vi[k] = t0; Vj[k] = t1; }
            }
        }
        if (!changed) break;
    }
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sqrt(sd);
    }
    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            { const double t = W[i]; W[i] = W[j]; W[j] = t; }
            for (k = 0; k < m; k++) { const double t = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = t; }
            if (wantV) for (k = 0; k < n; k++) { const double t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
        }
    }
    for (i = 0; i < n; i++) Wout[i] = W[i];
    uint64_t rng = 0x12345678;
    for (i = 0; i < n1; i++) {
        sd = i < n ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const double val0 = 1. / m;
            for (k = 0; k < m; k++) {
                rng = (uint64_t)(uint32_t)rng * 4164903690U + (uint32_t)(rng >> 32);
                At[i * m + k] = ((uint32_t)rng & 256) != 0 ? val0 : -val0;
            }
            for (iter = 0; iter < 2; iter++) {
                for (j = 0; j < i; j++) {
                    sd = 0;
                    for (k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    double asum = 0;
                    for (k = 0; k < m; k++) { const double t = At[i * m + k] - sd * At[j * m + k]; At[i * m + k] = t; asum += fabs(t); }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (k = 0; k < m; k++) At[i * m + k] *= asum;
                }
                sd = 0;
                for (k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
                sd = sqrt(sd);
            }
        }
        s = sd > minval ? 1 / sd : 0.;
        for (k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

// cvSolve(A [6][nc], b [6], x [nc], CV_SVD), nc <= 5
SIND_HD inline void epnp_solve_svd(const double* A, int nc, const double* b, double* x) {
    double At[5 * 6], W[5], Vt[5 * 5];
    for (int i = 0; i < nc; i++) for (int k = 0; k < 6; k++) At[i * 6 + k] = A[k * nc + i];
    epnp_jacobi_svd(At, W, Vt, true, 6, nc, nc);
    double threshold = 0;
    for (int j = 0; j < nc; j++) x[j] = 0;
    for (int i = 0; i < nc; i++) threshold += W[i];
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < nc; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < 6; j++) s += At[i * 6 + j] * b[j];
        s *= wi;
        for (int j = 0; j < nc; j++) x[j] = x[j] + s * Vt[i * nc + j];
    }
}

// cvInvert(A, X, CV_SVD) of a 3 x 3
SIND_HD inline void epnp_invert3(const double* A, double* X) {
    double At[9], W[3], Vt[9], buffer[3];
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) At[i * 3 + k] = A[k * 3 + i];
    epnp_jacobi_svd(At, W, Vt, true, 3, 3, 3);
    double threshold = 0;
    for (int j = 0; j < 9; j++) X[j] = 0;
    for (int i = 0; i < 3; i++) threshold += W[i];
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < 3; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        for (int j = 0; j < 3; j++) buffer[j] = At[i * 3 + j] * wi;                                  // U[j][i] = At[i][j]
        for (int r = 0; r < 3; r++) { const double sv = Vt[i * 3 + r]; for (int j = 0; j < 3; j++) X[r * 3 + j] = X[r * 3 + j] + sv * buffer[j]; }
    }
}

SIND_HD inline double epnp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SIND_HD inline double epnp_dist2(const double* p1, const double* p2) {
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

// qr_solve (:860-950) of the 6 x 4 system; A and b are overwritten
SIND_HD inline void epnp_qr_solve(double* pA, double* pb, double* pX) {
    const int nr = 6, nc = 4;
    double A1[6], A2[6];
    double* ppAkk = pA;
    for (int k = 0; k < nc; k++) {
        double* ppAik = ppAkk; double eta = fabs(*ppAik);
        for (int i = k + 1; i < nr; i++) { const double elt = fabs(*ppAik); if (eta < elt) eta = elt; ppAik += nc; }   // as written there: rows k .. nr - 2
        if (eta == 0) { A1[k] = A2[k] = 0.0; return; }
        {
            double* q = ppAkk; double sum = 0.0; const double inv_eta = 1. / eta;
            for (int i = k; i < nr; i++) { *q *= inv_eta; sum += *q * *q; q += nc; }
            double sigma = sqrt(sum);
            if (*ppAkk < 0) sigma = -sigma;
            *ppAkk += sigma;
            A1[k] = sigma * *ppAkk;
            A2[k] = -eta * sigma;
            for (int j = k + 1; j < nc; j++) {
                double* r = ppAkk; double sm = 0;
                for (int i = k; i < nr; i++) { sm += *r * r[j - k]; r += nc; }
                const double tau = sm / A1[k];
                r = ppAkk;
                for (int i = k; i < nr; i++) { r[j - k] -= tau * *r; r += nc; }
            }
        }
        ppAkk += nc + 1;
    }
    double* ppAjj = pA;
    for (int j = 0; j < nc; j++) {
        double* ppAij = ppAjj; double tau = 0;
        for (int i = j; i < nr; i++) { tau += *ppAij * pb[i]; ppAij += nc; }
        tau /= A1[j];
        ppAij = ppAjj;
        for (int i = j; i < nr; i++) { pb[i] -= tau * *ppAij; ppAij += nc; }
        ppAjj += nc + 1;
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        const double* ppAij = pA + i * nc + (i + 1); double sum = 0;
        for (int j = i + 1; j < nc; j++) { sum += *ppAij * pX[j]; ppAij++; }
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838)
SIND_HD inline void epnp_gauss_newton(const double* l_6x10, const double* rho, double betas[4]) {
    double a[6 * 4], b[6], x[4] = {0, 0, 0, 0};
    for (int k = 0; k < 5; k++) {
        for (int i = 0; i < 6; i++) {
            const double* rowL = l_6x10 + i * 10; double* rowA = a + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                             rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                             rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
        }
        epnp_qr_solve(a, b, x);
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// find_betas_approx_1 / 2 / 3 (:667-758)
SIND_HD inline void epnp_find_betas(int which, const double* l_6x10, const double* rho, double* betas) {
    const int nc = which == 1 ? 4 : which == 2 ? 3 : 5;
    const int col1[4] = {0, 1, 3, 6};
    double l[6 * 5], b[5];
    for (int i = 0; i < 6; i++) for (int j = 0; j < nc; j++) l[i * nc + j] = l_6x10[i * 10 + (which == 1 ? col1[j] : j)];
    epnp_solve_svd(l, nc, rho, b);
    if (which == 1) {
        if (b[0] < 0) { betas[0] = sqrt(-b[0]); betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0]; }
        else { betas[0] = sqrt(b[0]); betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0]; }
        return;
    }
    if (b[0] < 0) { betas[0] = sqrt(-b[0]); betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0; }
    else { betas[0] = sqrt(b[0]); betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0; }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = which == 2 ? 0.0 : b[3] / betas[0];
    betas[3] = 0.0;
}

// the n-sized arrays: element k of an array lives at [k * S] (S = 1 on the host; on the device the lanes of a wave interleave their problems)
#define EPNP_AT(a, k) a[(size_t)(k) * S]

// compute_R_and_t (:651-662): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
SIND_HD inline double epnp_R_and_t(int n, const double* pws, const double* us, const double* alphas, double* pcs, int S, double fu, double fv, double uc, double vc,
                                   const double* ut, const double* betas, double R[3][3], double t[3]) {
    double ccs[4][3];
    for (int i = 0; i < 4; i++) ccs[i][0] = ccs[i][1] = ccs[i][2] = 0.0f;
    for (int i = 0; i < 4; i++) {
        const double* v = ut + 12 * (11 - i);
        for (int j = 0; j < 4; j++) for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[3 * j + k];
    }
    for (int i = 0; i < n; i++) {
        const double a0 = EPNP_AT(alphas, 4 * i), a1 = EPNP_AT(alphas, 4 * i + 1), a2 = EPNP_AT(alphas, 4 * i + 2), a3 = EPNP_AT(alphas, 4 * i + 3);
        for (int j = 0; j < 3; j++) EPNP_AT(pcs, 3 * i + j) = a0 * ccs[0][j] + a1 * ccs[1][j] + a2 * ccs[2][j] + a3 * ccs[3][j];
    }
    if (EPNP_AT(pcs, 2) < 0.0) {                                                                      // solve_for_sign; ccs is not read again
        for (int i = 0; i < n; i++) for (int j = 0; j < 3; j++) EPNP_AT(pcs, 3 * i + j) = -EPNP_AT(pcs, 3 * i + j);
    }
    // estimate_R_and_t (:569-627)
    double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
    for (int i = 0; i < n; i++) for (int j = 0; j < 3; j++) { pc0[j] += EPNP_AT(pcs, 3 * i + j); pw0[j] += EPNP_AT(pws, 3 * i + j); }
    for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
    double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
        const double w0 = EPNP_AT(pws, 3 * i), w1 = EPNP_AT(pws, 3 * i + 1), w2 = EPNP_AT(pws, 3 * i + 2);
        for (int j = 0; j < 3; j++) {
            const double pc = EPNP_AT(pcs, 3 * i + j);
            abt[3 * j] += (pc - pc0[j]) * (w0 - pw0[0]);
            abt[3 * j + 1] += (pc - pc0[j]) * (w1 - pw0[1]);
            abt[3 * j + 2] += (pc - pc0[j]) * (w2 - pw0[2]);
        }
    }
    double At[9], D[3], Vt[9], abt_u[9], abt_v[9];                                                    // cvSVD(&ABt, &ABt_D, &ABt_U, &ABt_V, CV_SVD_MODIFY_A)
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) At[i * 3 + k] = abt[k * 3 + i];
    epnp_jacobi_svd(At, D, Vt, true, 3, 3, 3);
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) { abt_u[3 * i + k] = At[3 * k + i]; abt_v[3 * i + k] = Vt[3 * k + i]; }
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = epnp_dot(abt_u + 3 * i, abt_v + 3 * j);
    const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
                       R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
    if (det < 0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
    t[0] = pc0[0] - epnp_dot(R[0], pw0); t[1] = pc0[1] - epnp_dot(R[1], pw0); t[2] = pc0[2] - epnp_dot(R[2], pw0);
    // reprojection_error (:550-567)
    double sum2 = 0.0;
    for (int i = 0; i < n; i++) {
        const double pw[3] = {EPNP_AT(pws, 3 * i), EPNP_AT(pws, 3 * i + 1), EPNP_AT(pws, 3 * i + 2)};
        const double Xc = epnp_dot(R[0], pw) + t[0], Yc = epnp_dot(R[1], pw) + t[1], inv_Zc = 1.0 / (epnp_dot(R[2], pw) + t[2]);
        const double ue = uc + fu * Xc * inv_Zc, ve = vc + fv * Yc * inv_Zc;
        const double u = EPNP_AT(us, 2 * i), v = EPNP_AT(us, 2 * i + 1);
        sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    return sum2 / n;
}

// compute_pose (:477-525) on n correspondences.  pws [3 n], us [2 n] in; workspace: alphas [4 n] then pcs [3 n] (7 n elements); all four strided by S.
// mtm: 144 doubles of scratch the caller places (the 12 x 12 matrix the SVD rotates in place; it is U^T afterwards).  -> the reprojection error it returns
SIND_HD inline double epnp_compute_pose(int n, const double* pws, const double* us, int S, double fu, double fv, double uc, double vc, double* workspace, double* mtm,
                                        double R[3][3], double t[3]) {
    double* alphas = workspace; double* pcs = workspace + (size_t)4 * n * S;
    // choose_control_points (:375-409)
    double cws[4][3];
    cws[0][0] = cws[0][1] = cws[0][2] = 0;
    for (int i = 0; i < n; i++) for (int j = 0; j < 3; j++) cws[0][j] += EPNP_AT(pws, 3 * i + j);
    for (int j = 0; j < 3; j++) cws[0][j] /= n;
    {
        double pw0tpw0[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dc[3];
        for (int k = 0; k < n; k++) {
            double row[3]; for (int j = 0; j < 3; j++) row[j] = EPNP_AT(pws, 3 * k + j) - cws[0][j];
            for (int i = 0; i < 3; i++) for (int j = i; j < 3; j++) pw0tpw0[3 * i + j] += row[i] * row[j];
        }
        for (int i = 0; i < 3; i++) for (int j = i; j < 3; j++) { pw0tpw0[3 * i + j] = pw0tpw0[3 * i + j] * 1.0; pw0tpw0[3 * j + i] = pw0tpw0[3 * i + j]; }
        epnp_jacobi_svd(pw0tpw0, dc, nullptr, false, 3, 3, 3);                                        // symmetric: At = A; CV_SVD_U_T: uct = At
        for (int i = 1; i < 4; i++) {
            const double k = sqrt(dc[i - 1] / n);
            for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * pw0tpw0[3 * (i - 1) + j];
        }
    }
    // compute_barycentric_coordinates (:411-434)
    {
        double cc[9], ci[9];
        for (int i = 0; i < 3; i++) for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
        epnp_invert3(cc, ci);
        for (int i = 0; i < n; i++) {
            const double p0 = EPNP_AT(pws, 3 * i), p1 = EPNP_AT(pws, 3 * i + 1), p2 = EPNP_AT(pws, 3 * i + 2);
            double a[4];
            for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * (p0 - cws[0][0]) + ci[3 * j + 1] * (p1 - cws[0][1]) + ci[3 * j + 2] * (p2 - cws[0][2]);
            a[0] = 1.0f - a[1] - a[2] - a[3];
            for (int j = 0; j < 4; j++) EPNP_AT(alphas, 4 * i + j) = a[j];
        }
    }
    // fill_M (:436-451) and cvMulTransposed(M, &MtM, 1): M's rows are formed one pair at a time and added to the upper triangle, row index ascending
    for (int i = 0; i < 144; i++) mtm[i] = 0;
    for (int i = 0; i < n; i++) {
        double M1[12], M2[12];
        const double u = EPNP_AT(us, 2 * i), v = EPNP_AT(us, 2 * i + 1);
        for (int c = 0; c < 4; c++) {
            const double as = EPNP_AT(alphas, 4 * i + c);
            M1[3 * c] = as * fu; M1[3 * c + 1] = 0.0; M1[3 * c + 2] = as * (uc - u);
            M2[3 * c] = 0.0; M2[3 * c + 1] = as * fv; M2[3 * c + 2] = as * (vc - v);
        }
        for (int a = 0; a < 12; a++) for (int b = a; b < 12; b++) mtm[12 * a + b] += M1[a] * M1[b];
        for (int a = 0; a < 12; a++) for (int b = a; b < 12; b++) mtm[12 * a + b] += M2[a] * M2[b];
    }
    for (int a = 0; a < 12; a++) for (int b = a; b < 12; b++) { mtm[12 * a + b] = mtm[12 * a + b] * 1.0; mtm[12 * b + a] = mtm[12 * a + b]; }
    double d[12];
    epnp_jacobi_svd(mtm, d, nullptr, false, 12, 12, 12);                                              // cvSVD(&MtM, &D, &Ut, 0, CV_SVD_MODIFY_A | CV_SVD_U_T): ut = At
    const double* ut = mtm;
    // compute_L_6x10 (:760-800), compute_rho (:802-810)
    double l_6x10[60], rho[6];
    {
        double dv[4][6][3];
        for (int i = 0; i < 4; i++) {
            const double* v = ut + 12 * (11 - i);
            int a = 0, b = 1;
            for (int j = 0; j < 6; j++) {
                dv[i][j][0] = v[3 * a] - v[3 * b]; dv[i][j][1] = v[3 * a + 1] - v[3 * b + 1]; dv[i][j][2] = v[3 * a + 2] - v[3 * b + 2];
                b++;
                if (b > 3) { a++; b = a + 1; }
            }
        }
        for (int i = 0; i < 6; i++) {
            double* row = l_6x10 + 10 * i;
            row[0] = epnp_dot(dv[0][i], dv[0][i]);
            row[1] = 2.0f * epnp_dot(dv[0][i], dv[1][i]);
            row[2] = epnp_dot(dv[1][i], dv[1][i]);
            row[3] = 2.0f * epnp_dot(dv[0][i], dv[2][i]);
            row[4] = 2.0f * epnp_dot(dv[1][i], dv[2][i]);
            row[5] = epnp_dot(dv[2][i], dv[2][i]);
            row[6] = 2.0f * epnp_dot(dv[0][i], dv[3][i]);
            row[7] = 2.0f * epnp_dot(dv[1][i], dv[3][i]);
            row[8] = 2.0f * epnp_dot(dv[2][i], dv[3][i]);
            row[9] = epnp_dot(dv[3][i], dv[3][i]);
        }
    }
    rho[0] = epnp_dist2(cws[0], cws[1]); rho[1] = epnp_dist2(cws[0], cws[2]); rho[2] = epnp_dist2(cws[0], cws[3]);
    rho[3] = epnp_dist2(cws[1], cws[2]); rho[4] = epnp_dist2(cws[1], cws[3]); rho[5] = epnp_dist2(cws[2], cws[3]);
    double Betas[4][4], rep_errors[4], Rs[4][3][3], ts[4][3];
    for (int w = 1; w <= 3; w++) {
        epnp_find_betas(w, l_6x10, rho, Betas[w]);
        epnp_gauss_newton(l_6x10, rho, Betas[w]);
        rep_errors[w] = epnp_R_and_t(n, pws, us, alphas, pcs, S, fu, fv, uc, vc, ut, Betas[w], Rs[w], ts[w]);
    }
    int N = 1;
    if (rep_errors[2] < rep_errors[1]) N = 2;
    if (rep_errors[3] < rep_errors[N]) N = 3;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R[i][j] = Rs[N][i][j]; t[i] = ts[N][i]; }
    return rep_errors[N];
}
#undef EPNP_AT

// CheckInliers (:308-339) for one correspondence: P3Dw, P2D FP32, the pose FP64, maxError = mvSigma2[i] * th2 FP32
SIND_HD inline bool epnp_is_inlier(const double* R /* 9 */, const double* t, double fu, double fv, double uc, double vc, float X, float Y, float Z, float u, float v, float maxError) {
    const float Xc = (float)(R[0] * X + R[1] * Y + R[2] * Z + t[0]);
    const float Yc = (float)(R[3] * X + R[4] * Y + R[5] * Z + t[1]);
    const float invZc = (float)(1 / (R[6] * X + R[7] * Y + R[8] * Z + t[2]));
    const double ue = uc + fu * Xc * invZc, ve = vc + fv * Yc * invZc;
    const float distX = (float)(u - ue), distY = (float)(v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < maxError;
}

}  // namespace sind
