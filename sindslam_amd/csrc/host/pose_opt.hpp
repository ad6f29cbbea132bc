// Optimizer::PoseOptimization (reference src/Optimizer.cc:239-451) written out: one 6-DoF vertex, N unary reprojection edges (mono or stereo), Levenberg-Marquardt
// on a dense 6 x 6 system, four rounds of ten iterations with outliers reclassified in between.  ONE source for the host (libsind_host.so: sindh_pose_optimize,
// pose_opt.cpp) and the device (../match_pose.hip: k_pose_opt), as epnp.hpp is: IEEE FP64 add / mul / div / sqrt on both sides and no contraction
// (-ffp-contract=off), so the two give the same bits.  The control flow (pose_optimize) is a template over an evaluator that owns the edges: the host's is the plain
// sequential loop, the device's has the lanes of a workgroup stride over the edges and 28 lanes add the contributions in ascending edge order.
//
// UNPINNED PARITY.  g2o and Eigen are not available to build or run; what follows is restated from the reference's Thirdparty/g2o and from Eigen 3.3 as remembered.
//   1. Eigen's evaluation order inside the small products (A^T Omega A, A^T Omega e, e^T Omega e, Omega * Omega, V * upsilon, the quaternion product and rotation, the
//      norm of a quaternion).  DEFINED here: every sum in ascending index order, Omega = invSigma2 * I applied as one multiplication per row (no products with the
//      zeros off its diagonal: with an infinite error Eigen's 0 * inf would give NaN where this gives inf).
//   2. The reference builds with -march=native, so its compiler may contract a * b + c; here nothing is contracted.
//   3. Two definitions that replace maths-library calls: po_sincos for sin(theta) and cos(theta) of SE3Quat::exp (Cody-Waite reduction by pi/2 in fdlibm's
//      second-iteration form, fdlibm / FreeBSD msun kernel polynomials; only add, mul, div, rint, compares; NaN gives NaN, 0 gives exactly 0 and 1; accurate below
//      |theta| of about 2^20 pi/2, beyond it still total and the same on both sides), and pow(theta, 3) as x * x * x.
//   4. What g2o_lm.hpp lists: Eigen's LDLT and the Levenberg-Marquardt control flow, shared with sim3_opt.hpp and local_ba.hpp.
// Of g2o_lm.hpp's literal points, here: the solver's x is kept across iterations AND rounds, as the BlockSolver keeps it; and after a round whose last trial was
// rejected the level-0 edges are classified with the REJECTED pose (their stored errors) and only the former outliers (computeError, :388-391) with the restored one.
#pragma once
#include <cstddef>
#include <cstdint>
#include "g2o_lm.hpp"                                                // SIND_HD; the LDLT and the Levenberg-Marquardt driver

struct sind_poseopt_item;

namespace sind {

struct PoseQ { double q[4] /* x y z w, Eigen's coeffs() */, t[3]; };                 // g2o::SE3Quat
struct PoseOptCam { double fx, fy, cx, cy, bf; };                                     // e->fx = pFrame->fx ...: the FP64 of FP32
struct PoseOptOut {                                                                   // everything the C ABI returns besides mvbOutlier
    float Tcw[16]; int nGood, nRounds, iters[4], nbad[4]; double pose[4][12], chi2[4], lambda[4];
};
#define POSEOPT_ENTRIES 28                                           // per edge: 21 of the upper triangle of A^T W A (row-major), 6 of A^T Omega e (rho[1] applied), rho[0]

// ---------------------------------------------------------------- sin and cos, defined (see 4. above)
SIND_HD inline void po_sincos(double x, double* s, double* c) {
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21;
    const double fn = __builtin_rint(x * invpio2);
    const double t = x - fn * pio2_1;                                // fdlibm e_rem_pio2.c, second iteration, taken always
    double w = fn * pio2_2;
    const double r = t - w;
    w = fn * pio2_2t - ((t - r) - w);
    const double y0 = r - w, y1 = (r - y0) - w;
    const double z = y0 * y0;
    // k_sin.c with iy = 1
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double v = z * y0, rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double ks = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1);
    // k_cos.c (FreeBSD msun form: no bit tricks)
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double hz = 0.5 * z, wc = 1.0 - hz;
    const double kc = wc + (((1.0 - wc) - hz) + (z * rc - y0 * y1));
    const double q = fn - 4.0 * __builtin_rint(fn * 0.25);           // fn mod 4 in {-2, -1, 0, 1, 2}; a NaN fails every compare and takes the last branch with NaN values
    if (q == 0.0) { *s = ks; *c = kc; }
    else if (q == 1.0) { *s = kc; *c = -ks; }
    else if (q == -1.0) { *s = -kc; *c = ks; }
    else { *s = -ks; *c = -kc; }
}

// ---------------------------------------------------------------- Eigen's quaternion
SIND_HD inline void po_quat_from_matrix(const double m[3][3], double q[4]) {          // Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0.0) {
        t = sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[k][j] - m[j][k]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[k] = (m[k][i] + m[i][k]) * t;
    }
}
SIND_HD inline void po_quat_to_matrix(const double q[4], double m[3][3]) {            // QuaternionBase::toRotationMatrix
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    m[0][0] = 1.0 - (tyy + tzz); m[0][1] = txy - twz; m[0][2] = txz + twy;
    m[1][0] = txy + twz; m[1][1] = 1.0 - (txx + tzz); m[1][2] = tyz - twx;
    m[2][0] = txz - twy; m[2][1] = tyz + twx; m[2][2] = 1.0 - (txx + tyy);
}
SIND_HD inline void po_quat_rotate(const double q[4], const double v[3], double out[3]) {   // QuaternionBase::_transformVector: uv = 2 vec x v; v + w uv + vec x uv
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    out[0] = v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]);
    out[1] = v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]);
    out[2] = v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0]);
}
// SE3Quat::normalizeRotation (se3quat.h:280-285): w < 0 flips, then Quaternion::normalize = coeffs / norm
SIND_HD inline void po_normalize_rotation(double q[4]) {
    if (q[3] < 0.0) { q[0] *= -1.0; q[1] *= -1.0; q[2] *= -1.0; q[3] *= -1.0; }
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= nrm; q[1] /= nrm; q[2] /= nrm; q[3] /= nrm;
}
// SE3Quat(const Matrix3d& R, const Vector3d& t) (se3quat.h:58-60)
SIND_HD inline void po_se3(const double R[3][3], const double t[3], PoseQ& P) {
    po_quat_from_matrix(R, P.q); P.t[0] = t[0]; P.t[1] = t[1]; P.t[2] = t[2];
    po_normalize_rotation(P.q);
}
// Converter::toSE3Quat (src/Converter.cc:37-47): the FP32 of mTcw read as FP64
SIND_HD inline void po_from_tcw(const float* T, PoseQ& P) {
    double R[3][3], t[3];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R[i][j] = (double)T[4 * i + j]; t[i] = (double)T[4 * i + 3]; }
    po_se3(R, t, P);
}
// Converter::toCvMat(SE3Quat) (src/Converter.cc:49-53, :63-71): to_homogeneous_matrix (se3quat.h:270-278) cast to float
SIND_HD inline void po_to_tcw(const PoseQ& P, float* T) {
    double R[3][3]; po_quat_to_matrix(P.q, R);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[i][j]; T[4 * i + 3] = (float)P.t[i]; }
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}
// SE3Quat::map (se3quat.h:217-220): _r * xyz + _t
SIND_HD inline void po_map(const PoseQ& P, const double X[3], double out[3]) {
    double r[3]; po_quat_rotate(P.q, X, r);
    out[0] = r[0] + P.t[0]; out[1] = r[1] + P.t[1]; out[2] = r[2] + P.t[2];
}
// SE3Quat::exp (se3quat.h:223-257), with the theta < 0.00001 branch as written (R = I + Omega + Omega^2, V = R)
SIND_HD inline void po_exp(const double u[6], PoseQ& P) {
    const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};   // skew (se3_ops.hpp)
    double O2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    if (theta < 0.00001) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j]; V[i][j] = R[i][j]; }
    } else {
        double s, c; po_sincos(theta, &s, &c);
        const double a = s / theta, b = (1.0 - c) / (theta * theta), d = (theta - s) / (theta * theta * theta);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
            const double I = i == j ? 1.0 : 0.0;
            R[i][j] = (I + a * O[i][j]) + b * O2[i][j];
            V[i][j] = (I + b * O[i][j]) + d * O2[i][j];
        }
    }
    double t[3];
    for (int i = 0; i < 3; i++) t[i] = V[i][0] * up[0] + V[i][1] * up[1] + V[i][2] * up[2];
    po_quat_from_matrix(R, P.q); P.t[0] = t[0]; P.t[1] = t[1]; P.t[2] = t[2];                   // SE3Quat(Quaterniond(R), V * upsilon)
    po_normalize_rotation(P.q);
}
// SE3Quat::operator* (se3quat.h:104-110): t = a.t + a.r * b.t, r = a.r * b.r (Eigen's quaternion product), normalizeRotation
SIND_HD inline void po_mul(const PoseQ& A, const PoseQ& B, PoseQ& out) {
    double rt[3]; po_quat_rotate(A.q, B.t, rt);
    PoseQ r;
    r.t[0] = A.t[0] + rt[0]; r.t[1] = A.t[1] + rt[1]; r.t[2] = A.t[2] + rt[2];
    po_quat_mul(A.q, B.q, r.q);
    po_normalize_rotation(r.q);
    out = r;
}
// VertexSE3Expmap::oplusImpl (types_six_dof_expmap.h:64-67): setEstimate(SE3Quat::exp(update) * estimate())
SIND_HD inline void po_oplus(const double u[6], PoseQ& est) { PoseQ e; po_exp(u, e); po_mul(e, est, est); }

// ---------------------------------------------------------------- the two edges (types_six_dof_expmap.h / .cpp:266-364)
// computeError: obs - cam_project(estimate.map(Xw)); uR < 0 is the monocular edge.  -> chi2() = error . (information * error), information = invSigma2 I
SIND_HD inline double po_edge_error(const PoseQ& P, const PoseOptCam& K, const double X[3], double ox, double oy, double uR, bool stereo, double s, double e[3], double Xc[3]) {
    po_map(P, X, Xc);
    if (!stereo) {                                                   // EdgeSE3ProjectXYZOnlyPose::cam_project (:290-296) over project2d
        const double px = Xc[0] / Xc[2], py = Xc[1] / Xc[2];
        e[0] = ox - (px * K.fx + K.cx); e[1] = oy - (py * K.fy + K.cy); e[2] = 0.0;
        return e[0] * (s * e[0]) + e[1] * (s * e[1]);
    }
    const float invzf = (float)(1.0 / Xc[2]);                        // EdgeStereoSE3ProjectXYZOnlyPose::cam_project (:299-306): const float invz = 1.0f/trans_xyz[2]
    const double invz = (double)invzf;
    const double r0 = Xc[0] * invz * K.fx + K.cx, r1 = Xc[1] * invz * K.fy + K.cy, r2 = r0 - K.bf * invz;
    e[0] = ox - r0; e[1] = oy - r1; e[2] = uR - r2;
    return e[0] * (s * e[0]) + e[1] * (s * e[1]) + e[2] * (s * e[2]);
}
// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91); rho[2] is computed there and used nowhere (robustInformation's second-order term is commented out)
SIND_HD inline void po_huber(double e, double delta, double* rho0, double* rho1) {
    const double dsqr = delta * delta;
    if (e <= dsqr) { *rho0 = e; *rho1 = 1.0; }
    else { const double sqrte = sqrt(e); *rho0 = 2 * sqrte * delta - dsqr; *rho1 = delta / sqrte; }
}
SIND_HD inline double po_delta(bool stereo) { return stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991); }   // const float deltaMono = sqrt(5.991), deltaStereo = sqrt(7.815) (:273-274); setDelta takes a double
// One edge of computeActiveErrors + activeRobustChi2 (+ linearizeOplus + constructQuadraticForm if full) at pose P.  c [28]: see POSEOPT_ENTRIES; not full: only c[27]
SIND_HD inline void po_edge_contrib(const PoseQ& P, const PoseOptCam& K, float Xx, float Xy, float Xz, float oxf, float oyf, float uRf, float invSigma2, bool robust, bool full, double* c) {
    const bool stereo = !(uRf < 0.0f);                               // if(pFrame->mvuRight[i]<0) mono, else stereo (:286, :320)
    const double X[3] = {(double)Xx, (double)Xy, (double)Xz}, s = (double)invSigma2;
    double e[3], Xc[3];
    const double chi2 = po_edge_error(P, K, X, (double)oxf, (double)oyf, (double)uRf, stereo, s, e, Xc);
    double rho0 = chi2, rho1 = 1.0;
    if (robust) po_huber(chi2, po_delta(stereo), &rho0, &rho1);
    c[27] = rho0;                                                    // activeRobustChi2: rho[0] with a kernel, chi2() without
    if (!full) return;
    const double x = Xc[0], y = Xc[1], invz = 1.0 / Xc[2], invz_2 = invz * invz;
    double A[3][6];
    A[0][0] = x * y * invz_2 * K.fx; A[0][1] = -(1 + (x * x * invz_2)) * K.fx; A[0][2] = y * invz * K.fx; A[0][3] = -invz * K.fx; A[0][4] = 0; A[0][5] = x * invz_2 * K.fx;
    A[1][0] = (1 + y * y * invz_2) * K.fy; A[1][1] = -x * y * invz_2 * K.fy; A[1][2] = -x * invz * K.fy; A[1][3] = 0; A[1][4] = -invz * K.fy; A[1][5] = y * invz_2 * K.fy;
    if (stereo) {
        A[2][0] = A[0][0] - K.bf * y * invz_2; A[2][1] = A[0][1] + K.bf * x * invz_2; A[2][2] = A[0][2]; A[2][3] = A[0][3]; A[2][4] = 0; A[2][5] = A[0][5] - K.bf * invz_2;
    } else { for (int j = 0; j < 6; j++) A[2][j] = 0.0; }
    // constructQuadraticForm (base_unary_edge.hpp:55-67): weightedOmega = rho[1] * information; b -= rho[1] * A^T * omega * error
    const double W = robust ? rho1 * s : s;
    const double se[3] = {s * e[0], s * e[1], s * e[2]};
    jtwj_upper(A, W, stereo, c);
    for (int j = 0; j < 6; j++) {
        double t = A[0][j] * se[0] + A[1][j] * se[1];
        if (stereo) t = t + A[2][j] * se[2];
        c[21 + j] = robust ? rho1 * t : t;
    }
}
// the classification of :382-438 for one edge: `const float chi2 = e->chi2(); if(chi2>chi2Mono[it])`; a NaN compares false: inlier
SIND_HD inline bool po_edge_is_outlier(const PoseQ& P, const PoseOptCam& K, float Xx, float Xy, float Xz, float oxf, float oyf, float uRf, float invSigma2) {
    const bool stereo = !(uRf < 0.0f);
    const double X[3] = {(double)Xx, (double)Xy, (double)Xz};
    double e[3], Xc[3];
    const float chi2 = (float)po_edge_error(P, K, X, (double)oxf, (double)oyf, (double)uRf, stereo, (double)invSigma2, e, Xc);
    return chi2 > (stereo ? 7.815f : 5.991f);
}

// ---------------------------------------------------------------- the outer function over levenberg_optimize (g2o_lm.hpp)
// Ev: the edges of one frame.
//   void sums(const PoseQ& P, bool robust, bool full, double* S)   over the level-0 edges in ascending order, each S[k] a sequential FP64 sum from 0: S[27] += rho[0]
//                                                                  (computeActiveErrors + activeRobustChi2); full: S[0..20] += H entries, S[21..26] -= b terms (buildSystem)
//   int classify(const PoseQ& Perr, const PoseQ& Pest)             :382-438: level-0 edges judged at Perr (their stored error), former outliers at Pest; sets
//                                                                  mvbOutlier = level; -> nBad
// One round as levenberg_optimize's problem: the frame's vertex est over Ev's edges; errPose is the pose the edges' stored errors belong to
template <class Ev> struct PoseLm : DenseSystem<6> {
    Ev& ev; PoseQ& est; PoseQ& errPose; bool robust; PoseQ backup;
    SIND_HD PoseLm(Ev& ev_, PoseQ& est_, PoseQ& errPose_, bool robust_, double (&x_)[6]) : DenseSystem<6>(x_), ev(ev_), est(est_), errPose(errPose_), robust(robust_) {}
    SIND_HD double linearize() { double S[POSEOPT_ENTRIES]; ev.sums(est, robust, true, S); errPose = est; load(S); return S[27]; }
    SIND_HD void push() { backup = est; }
    SIND_HD void update() { po_oplus(x, est); }
    SIND_HD double chi2() { double T[POSEOPT_ENTRIES]; ev.sums(est, robust, false, T); errPose = est; return T[27]; }
    SIND_HD void pop() { est = backup; }
};
template <class Ev> SIND_HD inline void pose_optimize(Ev& ev, int n, const float* Tcw, PoseOptOut& o) {
    o.nGood = 0; o.nRounds = 0;
    for (int r = 0; r < 4; r++) { o.iters[r] = 0; o.nbad[r] = 0; o.chi2[r] = 0.0; o.lambda[r] = 0.0; for (int k = 0; k < 12; k++) o.pose[r][k] = 0.0; }
    for (int k = 0; k < 16; k++) o.Tcw[k] = Tcw[k];
    if (n < 3) return;                                               // :364-365, before SetPose
    PoseQ P0; po_from_tcw(Tcw, P0);
    PoseQ est = P0;
    double x[6] = {0, 0, 0, 0, 0, 0};
    int nBad = 0;
    for (int it = 0; it < 4; it++) {                                 // :374
        est = P0;                                                    // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)): the INPUT pose, every round
        PoseQ errPose = est;
        PoseLm<Ev> lm(ev, est, errPose, it < 3, x);                  // e->setRobustKernel(0) after round index 2 (:407, :436)
        o.iters[it] = levenberg_optimize(lm, 10, o.chi2[it], o.lambda[it]);
        { double R[3][3]; po_quat_to_matrix(est.q, R); for (int a = 0; a < 3; a++) { for (int c = 0; c < 3; c++) o.pose[it][3 * a + c] = R[a][c]; o.pose[it][9 + a] = est.t[a]; } }
        nBad = ev.classify(errPose, est);
        o.nbad[it] = nBad; o.nRounds = it + 1;
        if (n < 10) break;                                           // optimizer.edges().size()<10: all edges, not the active ones (:440)
    }
    po_to_tcw(est, o.Tcw);                                           // :445-448
    o.nGood = n - nBad;
}

// an item's outputs from o (pose_opt.cpp); n < 3: n_good and n_rounds only, the reference's `return 0` before SetPose
void poseopt_store(const ::sind_poseopt_item& q, const PoseOptOut& o, const uint8_t* outlier);
// -> 0, or what is wrong with the item: 1 a negative n, 2 a NULL array, 3 an inv_sigma2 that is negative or not finite, 4 a pose that is not finite
int poseopt_check(const ::sind_poseopt_item& q);

// the plain sequential evaluator (the host library's)
struct PoseOptSeq {
    int n; const float* x3Dw; const float* obs; const float* uR; const float* invSigma2; PoseOptCam K; uint8_t* outlier;
    void sums(const PoseQ& P, bool robust, bool full, double* S) {
        for (int k = 0; k < POSEOPT_ENTRIES; k++) S[k] = 0.0;
        double c[POSEOPT_ENTRIES];
        for (int i = 0; i < n; i++) {
            if (outlier[i]) continue;                                // initializeOptimization(0): level-0 edges only
            po_edge_contrib(P, K, x3Dw[3 * i], x3Dw[3 * i + 1], x3Dw[3 * i + 2], obs[2 * i], obs[2 * i + 1], uR[i], invSigma2[i], robust, full, c);
            if (full) { for (int k = 0; k < 21; k++) S[k] = S[k] + c[k]; for (int k = 21; k < 27; k++) S[k] = S[k] - c[k]; }
            S[27] = S[27] + c[27];
        }
    }
    int classify(const PoseQ& Perr, const PoseQ& Pest) {
        int nBad = 0;
        for (int i = 0; i < n; i++) {
            const bool out = po_edge_is_outlier(outlier[i] ? Pest : Perr, K, x3Dw[3 * i], x3Dw[3 * i + 1], x3Dw[3 * i + 2], obs[2 * i], obs[2 * i + 1], uR[i], invSigma2[i]);
            outlier[i] = out ? 1 : 0; nBad += out ? 1 : 0;
        }
        return nBad;
    }
};

}  // namespace sind
