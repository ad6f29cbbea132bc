// Host stage: Sim3Solver::ComputeSim3 (reference src/Sim3Solver.cc:226-337, Horn 1987) for one sampled triple, and SetRansacParameters (:114-138).
// The inlier test of every hypothesis runs on the device (../match_sim3.hip); this half stays here, see that file's header.
//
// PARITY UNPINNED.  The reference writes the solve as cv::Mat expressions; OpenCV is not available to build or run, so each primitive is restated from
// OpenCV 4.2.0 as remembered, in the reference's order and types.  A build of OpenCV with Eigen (HAVE_EIGEN) may route cv::eigen to
// Eigen::SelfAdjointEigenSolver instead of its own Jacobi: then the quaternion differs in the last bits and everything after it.  tests/sim3_ref.py is the
// same restatement in Python (bit equality BY CONSTRUCTION); tests/test_sim3_cpu.py also compares with an FP64 SVD solution that shares none of the guesses.
// [R] = recalled with confidence, [G] = guessed / uncertain.
//   cv::reduce(P, C, 1, CV_REDUCE_SUM)   32F -> 32F, work type float; per row a0 = p[0], a1 = p[1], a0 += p[2], a0 += a1: (p0 + p2) + p1            [R: the two accumulators; G: that
//                                        no SIMD path reorders three columns]
//   C = C / P.cols                       MatExpr with alpha = 1. / 3 (double), assigned by convertTo: c * (float)alpha + 0.0f in FP32                 [R]
//   Pr.col(i) = P.col(i) - C             cv::subtract in FP32                                                                                    [R]
//   M = Pr2 * Pr1.t()                    cv::gemm with GEMM_2_T: not the small-matrix path (it needs flags == 0); the generic kernel accumulates the
//                                        products in FP64, k ascending, and stores (float)(s * alpha), alpha = 1                                    [R, as match_handle.hpp camera_centre]
//   N11 .. N44                           FP32 expressions of M's elements, left to right, widened to double and narrowed again by Mat_<float> <<    [R]
//   cv::eigen(N, eval, evec)             symmetric 4x4 CV_32F -> JacobiImpl_<float>: V = I; the pivot is the off-diagonal element of largest magnitude, tracked
//                                        per row (indR) and per column (indC); stop at |p| <= FLT_EPSILON or after 30 n^2 rotations; y = (W[l] - W[k]) * 0.5,
//                                        t = |y| + hypot(p, y), s = hypot(p, t), c = t / s, s = p / s, t = (p / t) * p, signs by y < 0; rotations
//                                        v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c; eigenvalues sorted descending by selection, eigenvectors as rows     [R: the scheme and
//                                        the formulas; G: that nothing in it is vectorised or contracted]
//                                        (not a cyclic sweep: the 4.2.0 code as remembered picks the largest pivot every time)
//   hypot(a, b)                          OpenCV's own: a = |a|, b = |b|; a > b: b /= a, a * sqrt(1 + b * b); b > 0: a /= b, b * sqrt(1 + a * a); else 0     [R]
//   norm(vec)                            NORM_L2 of 3 floats: squares and their sum in FP64, in order, then sqrt                                         [R]
//   atan2(norm(vec), evec(0, 0))         FP64, libm                                                                                               [R]
//   vec = 2 * ang * vec / norm(vec)      MatExpr: alpha = (2 * ang) * (1. / norm) in FP64, assigned by convertTo: v * (float)alpha + 0.0f in FP32        [R: alpha; G: the scalar tail
//                                        of cvt_32f for three elements, without FMA]
//   cv::Rodrigues(vec, R)                FP64 inside: theta = sqrt(x*x + y*y + z*z); theta < DBL_EPSILON -> identity; c = cos, s = sin, c1 = 1 - c, r *= 1 / theta,
//                                        R = (c * I + c1 * r rT) + s * [r]x element by element, stored as float.  A NaN theta takes the general branch     [R]
//   P3 = R * Pr2                         small-matrix path of cv::gemm: FP32 row product a0*b0 + a1*b1 + a2*b2, then (float)(t * 1.0)                 [R, as match_device.hpp d_to_camera]
//   nom = Pr1.dot(P3)                    dotProd_32f over the 9 continuous elements: no SIMD block below 16, then the unrolled scalar loop in FP64:
//                                        r += p0 + p1 + p2 + p3; r += p4 + p5 + p6 + p7; r += p8                                                      [R: FP64; G: the grouping]
//   cv::pow(P3, 2, aux); den             power 2 is cv::multiply in FP32; den adds the floats in FP64, row-major                                       [R]
//   ms12i = nom / den                    FP64 division, stored in a float member                                                                  [R]
//   mt12i = O1 - ms12i * R * O2          one cv::gemm(R, O2, alpha = -(double)ms12i, O1, beta = 1): small-matrix path, (float)(t * alpha + o1 * beta)  [R: MatOp_GEMM::subtract folds it]
//   sR = ms12i * R                       convertTo / cv::add: r * s + 0.0f in FP32                                                                 [R]
//   sRinv = (1.0 / ms12i) * R.t()        transpose, then convertTo: r * (float)(1.0 / (double)s) + 0.0f                                            [R]
//   tinv = -sRinv * mt12i                cv::gemm(sRinv, t, alpha = -1): small-matrix path, (float)(t * -1.0)                                       [R]
#include <cmath>
#include <cfloat>
#include <algorithm>
#include "sim3.hpp"
#include "sind_hip.h"

namespace sind {
namespace {

// ComputeCentroid (:215-224)
void centroid(const float* P, float* Pr, float* C) {
    const float third = (float)(1. / 3);
    for (int r = 0; r < 3; r++) {
        float a0 = P[3 * r], a1 = P[3 * r + 1];
        a0 = a0 + P[3 * r + 2]; a0 = a0 + a1;
        C[r] = a0 * third + 0.0f;
    }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Pr[3 * r + c] = P[3 * r + c] - C[r];
}

float cv_hypot(float a, float b) {
    a = std::fabs(a); b = std::fabs(b);
    if (a > b) { b /= a; return a * std::sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * std::sqrt(1 + a * a); }
    return 0;
}

// cv::eigen of a symmetric n x n float matrix: W descending, the eigenvectors the rows of V
template <int n> void cv_jacobi(float* A, float* W, float* V) {
    const float eps = FLT_EPSILON;
    int indR[n], indC[n], i, k, m; float mv = 0;
    for (i = 0; i < n; i++) { for (k = 0; k < n; k++) V[i * n + k] = 0; V[i * n + i] = 1; }
    auto scan_row = [&](int r) { for (m = r + 1, mv = std::fabs(A[n * r + m]), i = r + 2; i < n; i++) { const float val = std::fabs(A[n * r + i]); if (mv < val) mv = val, m = i; } indR[r] = m; };
    auto scan_col = [&](int c) { for (m = 0, mv = std::fabs(A[c]), i = 1; i < c; i++) { const float val = std::fabs(A[n * i + c]); if (mv < val) mv = val, m = i; } indC[c] = m; };
    for (k = 0; k < n; k++) { W[k] = A[(n + 1) * k]; if (k < n - 1) scan_row(k); if (k > 0) scan_col(k); }
    for (int iters = 0; iters < n * n * 30; iters++) {
        for (k = 0, mv = std::fabs(A[indR[0]]), i = 1; i < n - 1; i++) { const float val = std::fabs(A[n * i + indR[i]]); if (mv < val) mv = val, k = i; }
        int l = indR[k];
        for (i = 1; i < n; i++) { const float val = std::fabs(A[n * indC[i] + i]); if (mv < val) mv = val, k = indC[i], l = i; }
        const float p = A[n * k + l];
        if (std::fabs(p) <= eps) break;
        const float y = (float)((W[l] - W[k]) * 0.5);
        float t = std::fabs(y) + cv_hypot(p, y);
        float s = cv_hypot(p, t);
        const float c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        A[n * k + l] = 0;
        W[k] -= t; W[l] += t;
        float a0, b0;
#define SIM3_ROTATE(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
        for (i = 0; i < k; i++) SIM3_ROTATE(A[n * i + k], A[n * i + l]);
        for (i = k + 1; i < l; i++) SIM3_ROTATE(A[n * k + i], A[n * i + l]);
        for (i = l + 1; i < n; i++) SIM3_ROTATE(A[n * k + i], A[n * l + i]);
        for (i = 0; i < n; i++) SIM3_ROTATE(V[n * k + i], V[n * l + i]);
#undef SIM3_ROTATE
        for (int j = 0; j < 2; j++) { const int idx = j == 0 ? k : l; if (idx < n - 1) scan_row(idx); if (idx > 0) scan_col(idx); }
    }
    for (k = 0; k < n - 1; k++) {
        m = k; for (i = k + 1; i < n; i++) if (W[m] < W[i]) m = i;
        if (k != m) { std::swap(W[m], W[k]); for (i = 0; i < n; i++) std::swap(V[n * m + i], V[n * k + i]); }
    }
}

// cv::Rodrigues, rotation vector -> matrix
void cv_rodrigues(const float* rv, float* R) {
    double r[3] = {rv[0], rv[1], rv[2]};
    const double theta = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < DBL_EPSILON) { for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f; return; }
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    for (int i = 0; i < 3; i++) r[i] *= itheta;
    const double rrt[9] = {r[0] * r[0], r[0] * r[1], r[0] * r[2], r[0] * r[1], r[1] * r[1], r[1] * r[2], r[0] * r[2], r[1] * r[2], r[2] * r[2]};
    const double rx[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
    for (int i = 0; i < 9; i++) { const double e = (i % 4 == 0) ? 1. : 0.; R[i] = (float)((c * e + c1 * rrt[i]) + s * rx[i]); }
}

}  // namespace

void sim3_horn(const float* P1, const float* P2, bool fixScale, Sim3Hyp& h) {
    // Step 1: centroids and relative coordinates
    float Pr1[9], Pr2[9], O1[3], O2[3];
    centroid(P1, Pr1, O1); centroid(P2, Pr2, O2);
    // Step 2: M = Pr2 * Pr1^T
    float M[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)Pr2[3 * i + k] * (double)Pr1[3 * j + k]; M[3 * i + j] = (float)(s * 1.0); }
    // Step 3: N
    const double N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3], N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2],
                 N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7], N44 = -M[0] - M[4] + M[8];
    float N[16] = {(float)N11, (float)N12, (float)N13, (float)N14, (float)N12, (float)N22, (float)N23, (float)N24,
                   (float)N13, (float)N23, (float)N33, (float)N34, (float)N14, (float)N24, (float)N34, (float)N44};
    // Step 4: the eigenvector of the largest eigenvalue is the quaternion
    float eval[4], evec[16];
    cv_jacobi<4>(N, eval, evec);
    float vec[3] = {evec[1], evec[2], evec[3]};
    double nn = 0; for (int k = 0; k < 3; k++) nn += (double)vec[k] * (double)vec[k];
    const double nrm = std::sqrt(nn), ang = std::atan2(nrm, (double)evec[0]);
    const float a = (float)((2 * ang) * (1. / nrm));
    for (int k = 0; k < 3; k++) vec[k] = vec[k] * a + 0.0f;
    cv_rodrigues(vec, h.R12);
    // Step 5: rotate set 2
    const float* R = h.R12;
    float P3[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { const float t = R[3 * i] * Pr2[j] + R[3 * i + 1] * Pr2[3 + j] + R[3 * i + 2] * Pr2[6 + j]; P3[3 * i + j] = (float)((double)t * 1.0); }
    // Step 6: scale
    if (!fixScale) {
        double p[9]; for (int i = 0; i < 9; i++) p[i] = (double)Pr1[i] * P3[i];
        double nom = 0; nom += p[0] + p[1] + p[2] + p[3]; nom += p[4] + p[5] + p[6] + p[7]; nom += p[8];
        double den = 0; for (int i = 0; i < 9; i++) { const float sq = P3[i] * P3[i]; den += sq; }
        h.s12 = (float)(nom / den);
    } else h.s12 = 1.0f;
    // Step 7: translation
    const float s = h.s12;
    for (int r = 0; r < 3; r++) { const float t = R[3 * r] * O2[0] + R[3 * r + 1] * O2[1] + R[3 * r + 2] * O2[2]; h.t12[r] = (float)((double)t * -(double)s + (double)O1[r] * 1.0); }
    // Step 8: T12 = [sR | t], T21 = [sRinv | -sRinv t]
    const float is = (float)(1.0 / (double)s);
    for (int i = 0; i < 16; i++) h.T12[i] = h.T21[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { h.T12[4 * r + c] = R[3 * r + c] * s + 0.0f; h.T21[4 * r + c] = R[3 * c + r] * is + 0.0f; }
        h.T12[4 * r + 3] = h.t12[r];
    }
    for (int r = 0; r < 3; r++) { const float t = h.T21[4 * r] * h.t12[0] + h.T21[4 * r + 1] * h.t12[1] + h.T21[4 * r + 2] * h.t12[2]; h.T21[4 * r + 3] = (float)((double)t * -1.0); }
}

}  // namespace sind

extern "C" {

// test entry of libsind_host.so; also present in libsind_hip.so
void sindh_sim3_horn(const float* P1, const float* P2, int fix_scale, float* R12, float* t12, float* s12, float* T12, float* T21) {
    sind::Sim3Hyp h; sind::sim3_horn(P1, P2, fix_scale != 0, h);
    std::copy(h.R12, h.R12 + 9, R12); std::copy(h.t12, h.t12 + 3, t12); *s12 = h.s12; std::copy(h.T12, h.T12 + 16, T12); std::copy(h.T21, h.T21 + 16, T21);
}

// Sim3Solver::SetRansacParameters (:114-138): mRansacMaxIts for n correspondences; 0 where iterate reports bNoMore at once (:146)
int sind_sim3_iterations(int n, double probability, int min_inliers, int max_its) {
    if (n < min_inliers || n < 1) return 0;
    const float epsilon = (float)min_inliers / n;
    int nIterations;
    if (min_inliers == n) nIterations = 1;
    else {
        const double it = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
        nIterations = !(it < (double)max_its) ? max_its : it < 1 ? 1 : (int)it;                              // bounded first: the reference converts an unbounded double to int
    }
    return std::max(1, std::min(nIterations, max_its));
}

}  // extern "C"
