// Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1046-1241) written out: one 7-DoF Sim3 vertex, per correspondence two fixed points and two binary reprojection
// edges (EdgeSim3ProjectXYZ into camera 1, EdgeInverseSim3ProjectXYZ into camera 2) with Huber kernels, Levenberg-Marquardt on a dense 7 x 7 system, two stages (5
// iterations, the bad pairs removed, 5 or 10 more from where the first stage stopped).  ONE source for the host (libsind_host.so: sindh_sim3_optimize, sim3_opt.cpp) and
// the device (../match_sim3opt.hip: k_sim3_opt), as pose_opt.hpp is: IEEE FP64 add / mul / div / sqrt on both sides and no contraction (-ffp-contract=off), so the two
// give the same bits.  The control flow (sim3_optimize) is a template over an evaluator that owns the edges.  The quaternion helpers, po_sincos and po_huber are
// pose_opt.hpp's, unchanged.
//
// THE JACOBIAN IS NUMERIC, as in the reference: linearizeOplus of both edges is commented out (types_seven_dof_expmap.h:147, :169), so BaseBinaryEdge::linearizeOplus
// (base_binary_edge.hpp:131-205) runs: per dimension d, oplus(+1e-9 e_d), computeError, oplus(-1e-9 e_d), computeError, column = (1 / (2 * 1e-9)) * (e+ - e-).  The 14
// perturbed estimates Sim3(+-1e-9 e_d) * estimate and their inverses do not depend on the edge: s3_perturbed forms them once per linearisation (same arithmetic, same
// bits as once per edge).  oplusImpl writes update[6] = 0 into the caller's array when _fix_scale is set: column 6 is then exactly zero, and the solver's x[6] is
// zero when computeScale reads it.
//
// UNPINNED PARITY.  g2o and Eigen are not available to build or run; what follows is restated from the reference's Thirdparty/g2o and from Eigen 3.3 as remembered.
//   1. Eigen's evaluation order in Sim3(const Vector7d&) (sim3.h:70-142): R = I + a Omega + b Omega2 and W = A Omega + B Omega2 + C I.  DEFINED here: both left to
//      right, entry by entry, (I + a O) + b O2 and (A O + B O2) + C I with I's entries 1.0 and 0.0 multiplied as written.
//   2. Eigen's evaluation order inside the small products (Omega * Omega, W * upsilon, J^T Omega J, J^T omega_r, e^T Omega e, the quaternion product and rotation, the
//      norm of omega).  DEFINED as in pose_opt.hpp: every sum in ascending index order, Omega = invSigma2 * I applied as one multiplication per row.
//   3. What g2o_lm.hpp lists: Eigen's LDLT (here ldlt_solve<7>) and the Levenberg-Marquardt control flow, shared with pose_opt.hpp and local_ba.hpp.
//   4. The reference builds with -march=native, so its compiler may contract a * b + c; here nothing is contracted.
//   5. Maths-library calls: sin and cos are po_sincos; std::exp is s3_exp, DEFINED here: reduction x = k ln2 + r with k = rint(x / ln2) (ln2 split in two as in fdlibm's
//      e_exp.c), fdlibm's polynomial c = r - r^2 (P1 + ...), y = 1 - ((lo - r c / (2 - c)) - hi) for every k (fdlibm's separate k = 0 form is not used), then an exact
//      scaling by 2^k (ldexp).  Only add, mul, div, rint, compares and that scaling.  exp(0) = 1 exactly, NaN gives NaN, above 709.78 +inf, below -745.2 zero.
// Of g2o_lm.hpp's literal points, here: the solver's x is kept across iterations and across the two stages (Solver::resizeVector reallocates on growth only), and
// the classification reads the edges' STORED errors: those of the last evaluated estimate, which after a rejected trial is the rejected one.
// Kept literally: no quaternion is ever normalised (Sim3's constructors, operator* and inverse() do not), so its norm drifts; the second stage starts from the first
// stage's estimate with lambda re-initialised; with fewer than 10 pairs left after the first stage the function returns 0 and the Sim3 stays the input, the matches
// already nulled.  An empty graph (n = 0): initializeOptimization reports "Attempt to initialize an empty graph" and returns false, _ivMap stays empty, optimize
// returns -1 without touching anything, nBad = 0, 0 < 10: return 0.  A NaN chi2 compares false with th2: the pair stays.
#pragma once
#include "pose_opt.hpp"
#include "fd_exp.hpp"

struct sind_sim3opt_item;

namespace sind {

struct Sim3Q { double q[4] /* x y z w */, t[3], s; };                                // g2o::Sim3
struct Sim3Cam { double fx, fy, cx, cy; };                                            // _focal_length, _principle_point: the FP64 of FP32
struct Sim3OptOut { double q[4], t[3], s; int nIn, nBad, stages, iters[2]; double chi2[2], lambda[2]; };   // everything the C ABI returns besides removed[]
#define SIM3OPT_ENTRIES 36                                           // per edge: 28 of the upper triangle of J^T W J (row-major), 7 of J^T omega_r, rho[0]
#define SIM3OPT_TRANSFORMS 15                                        // the estimate, then +delta and -delta of dimension 0, of dimension 1, ...

// ---------------------------------------------------------------- exp, defined (see 5. above): s3_exp, in fd_exp.hpp since the occupancy map uses it too

// ---------------------------------------------------------------- g2o::Sim3 (sim3.h)
// Sim3(const Matrix3d& R, const Vector3d& t, double s) of LoopClosing.cc:296 over Converter::toMatrix3d / toVector3d: the FP32 read as FP64, Quaterniond(R) not normalised
SIND_HD inline void s3_from_input(float s, const float* R, const float* t, Sim3Q& S) {
    double m[3][3];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) m[i][j] = (double)R[3 * i + j]; S.t[i] = (double)t[i]; }
    po_quat_from_matrix(m, S.q); S.s = (double)s;
}
// Sim3(const Vector7d& update) (sim3.h:70-142), its four branches as written
SIND_HD inline void s3_exp7(const double u[7], Sim3Q& S) {
    const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]}, sigma = u[6];
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    const double s = s3_exp(sigma);
    double O2[3][3], R[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    const double eps = 0.00001;
    double A, B, C;
    bool small = theta < eps;
    double sn = 0.0, cs = 1.0;
    if (!small) po_sincos(theta, &sn, &cs);
    if (fabs(sigma) < eps) {
        C = 1;
        if (small) { A = 1. / 2.; B = 1. / 6.; }
        else { const double theta2 = theta * theta; A = (1 - cs) / (theta2); B = (theta - sn) / (theta2 * theta); }
    } else {
        C = (s - 1) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    if (small) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];      // I + Omega + Omega*Omega
    } else {
        const double ra = sn / theta, rb = (1 - cs) / (theta * theta);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + ra * O[i][j]) + rb * O2[i][j];
    }
    po_quat_from_matrix(R, S.q);                                     // r = Quaterniond(R): not normalised
    for (int i = 0; i < 3; i++) {
        double W[3];
        for (int j = 0; j < 3; j++) W[j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);
        S.t[i] = W[0] * up[0] + W[1] * up[1] + W[2] * up[2];
    }
    S.s = s;
}
// operator* (sim3.h:266-272): r = r * other.r, t = s * (r * other.t) + t, s = s * other.s
SIND_HD inline void s3_mul(const Sim3Q& A, const Sim3Q& B, Sim3Q& out) {
    double rt[3]; po_quat_rotate(A.q, B.t, rt);
    Sim3Q r;
    po_quat_mul(A.q, B.q, r.q);
    for (int i = 0; i < 3; i++) r.t[i] = A.s * rt[i] + A.t[i];
    r.s = A.s * B.s;
    out = r;
}
// inverse() (sim3.h:233-236): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
SIND_HD inline void s3_inverse(const Sim3Q& S, Sim3Q& out) {
    Sim3Q r;
    r.q[0] = -S.q[0]; r.q[1] = -S.q[1]; r.q[2] = -S.q[2]; r.q[3] = S.q[3];
    const double f = -1. / S.s, v[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
    po_quat_rotate(r.q, v, r.t);
    r.s = 1. / S.s;
    out = r;
}
// map (sim3.h:144-146): s * (r * xyz) + t
SIND_HD inline void s3_map(const Sim3Q& S, const double X[3], double out[3]) {
    double r[3]; po_quat_rotate(S.q, X, r);
    for (int i = 0; i < 3; i++) out[i] = S.s * r[i] + S.t[i];
}
// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): update[6] = 0 written into the caller's array, setEstimate(Sim3(update) * estimate())
SIND_HD inline void s3_oplus(double u[7], bool fixScale, Sim3Q& est) {
    if (fixScale) u[6] = 0;
    Sim3Q e; s3_exp7(u, e); s3_mul(e, est, est);
}
// transform k of a linearisation and its inverse: k = 0 the estimate, k = 1 + 2 d the estimate after oplus(+1e-9 e_d), k = 2 + 2 d after oplus(-1e-9 e_d)
SIND_HD inline void s3_perturbed(const Sim3Q& est, int k, bool fixScale, Sim3Q& S, Sim3Q& Sinv) {
    S = est;
    if (k > 0) {
        const double delta = 1e-9;
        double add[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        add[(k - 1) >> 1] = ((k - 1) & 1) ? -delta : delta;
        s3_oplus(add, fixScale, S);
    }
    s3_inverse(S, Sinv);                                             // EdgeInverseSim3ProjectXYZ::computeError: v1->estimate().inverse()
}

// ---------------------------------------------------------------- the two edges (types_seven_dof_expmap.h:130-171)
// computeError of either edge: obs - cam_map(project(T.map(X))); T is the estimate and X the point of camera 2 for EdgeSim3ProjectXYZ (cam_map1), the estimate's
// inverse and the point of camera 1 for EdgeInverseSim3ProjectXYZ (cam_map2).  -> chi2() with information = invSigma2 I
SIND_HD inline double s3_edge_error(const Sim3Q& T, const Sim3Cam& K, const double X[3], double ox, double oy, double s, double e[2]) {
    double Xc[3]; s3_map(T, X, Xc);
    const double px = Xc[0] / Xc[2], py = Xc[1] / Xc[2];
    e[0] = ox - (px * K.fx + K.cx); e[1] = oy - (py * K.fy + K.cy);
    return e[0] * (s * e[0]) + e[1] * (s * e[1]);
}
SIND_HD inline double s3_delta(float th2) { return (double)(float)sqrt((double)th2); }                  // const float deltaHuber = sqrt(th2) (:1095); setDelta takes a double
// One edge of computeActiveErrors + activeRobustChi2 (+ the numeric linearizeOplus + constructQuadraticForm if full).  T [15]: the transforms of s3_perturbed, the
// inverses for the inverse edge.  c [36]: see SIM3OPT_ENTRIES; not full: only c[35]
SIND_HD inline void s3_edge_contrib(const Sim3Q* T, const Sim3Cam& K, float Xx, float Xy, float Xz, float oxf, float oyf, float invSigma2, double delta, bool full, double* c) {
    const double X[3] = {(double)Xx, (double)Xy, (double)Xz}, ox = (double)oxf, oy = (double)oyf, s = (double)invSigma2;
    double e[2];
    const double chi2 = s3_edge_error(T[0], K, X, ox, oy, s, e);
    double rho0, rho1; po_huber(chi2, delta, &rho0, &rho1);
    c[35] = rho0;
    if (!full) return;
    const double scalar = 1.0 / (2 * 1e-9);
    double J[2][7];
    for (int d = 0; d < 7; d++) {
        double ep[2], em[2];
        s3_edge_error(T[1 + 2 * d], K, X, ox, oy, s, ep);
        s3_edge_error(T[2 + 2 * d], K, X, ox, oy, s, em);
        J[0][d] = scalar * (ep[0] - em[0]); J[1][d] = scalar * (ep[1] - em[1]);      // errorBak = e+; errorBak -= e-; col(d) = scalar * errorBak
    }
    // constructQuadraticForm (base_binary_edge.hpp:55-120), the point fixed: omega_r = -omega * error, *= rho[1]; b += B^T omega_r; A += B^T (rho[1] omega) B
    const double W = rho1 * s;
    double omr[2] = {-(s * e[0]), -(s * e[1])};
    omr[0] *= rho1; omr[1] *= rho1;
    jtwj_upper(J, W, false, c);
    for (int j = 0; j < 7; j++) c[28 + j] = J[0][j] * omr[0] + J[1][j] * omr[1];
}
// `e12->chi2()>th2 || e21->chi2()>th2` (:1193, :1227) for one pair at the estimate S the edges' errors were last computed with; th2 is the float promoted
SIND_HD inline bool s3_pair_is_bad(const Sim3Q& S, const Sim3Q& Sinv, const Sim3Cam& K1, const Sim3Cam& K2, const float* X1, const float* X2, const float* o1, const float* o2, float is1, float is2, float th2) {
    const double x1[3] = {(double)X1[0], (double)X1[1], (double)X1[2]}, x2[3] = {(double)X2[0], (double)X2[1], (double)X2[2]};
    double e[2];
    const double c12 = s3_edge_error(S, K1, x2, (double)o1[0], (double)o1[1], (double)is1, e);
    const double c21 = s3_edge_error(Sinv, K2, x1, (double)o2[0], (double)o2[1], (double)is2, e);
    return c12 > (double)th2 || c21 > (double)th2;
}

// ---------------------------------------------------------------- the outer function (:1180-1240) over levenberg_optimize (g2o_lm.hpp)
// Ev: the pairs of one item.
//   void sums(const Sim3Q& est, bool full, double* S)   over the edges of the pairs not removed, in insertion order (e12 of pair 0, e21 of pair 0, e12 of pair 1, ...:
//                                                       the active edges are sorted by internal id), each S[k] a sequential FP64 sum from 0: S[35] += rho[0];
//                                                       full: S[0..27] += H entries, S[28..34] += b terms, linearised at est
//   int classify(const Sim3Q& Serr, int* nIn)           :1186-1203 / :1220-1234 at the estimate of the stored errors: marks the pairs over th2 removed; -> how many it
//                                                       marked, *nIn = how many of the pairs it looked at stay
// Both stages as levenberg_optimize's problem: the Sim3 vertex est over Ev's edges; errS is the estimate the edges' stored errors belong to
template <class Ev> struct Sim3Lm : DenseSystem<7> {
    Ev& ev; Sim3Q& est; Sim3Q& errS; bool fixScale; Sim3Q backup;
    SIND_HD Sim3Lm(Ev& ev_, Sim3Q& est_, Sim3Q& errS_, bool fixScale_, double (&x_)[7]) : DenseSystem<7>(x_), ev(ev_), est(est_), errS(errS_), fixScale(fixScale_) {}
    SIND_HD double linearize() { double S[SIM3OPT_ENTRIES]; ev.sums(est, true, S); errS = est; load(S); return S[35]; }
    SIND_HD void push() { backup = est; }
    SIND_HD void update() { s3_oplus(x, fixScale, est); }            // x[6] = 0 stays in the solver's vector, where computeScale reads it
    SIND_HD double chi2() { double T[SIM3OPT_ENTRIES]; ev.sums(est, false, T); errS = est; return T[35]; }
    SIND_HD void pop() { est = backup; }
};
template <class Ev> SIND_HD inline void sim3_optimize(Ev& ev, int n, const Sim3Q& S0, bool fixScale, Sim3OptOut& o) {
    for (int k = 0; k < 4; k++) o.q[k] = S0.q[k];
    for (int k = 0; k < 3; k++) o.t[k] = S0.t[k];
    o.s = S0.s; o.nIn = 0; o.nBad = 0; o.stages = 0;
    for (int r = 0; r < 2; r++) { o.iters[r] = 0; o.chi2[r] = 0.0; o.lambda[r] = 0.0; }
    if (n < 1) return;                                               // the empty graph: see the head of this file
    Sim3Q est = S0, errS = S0;
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    Sim3Lm<Ev> lm(ev, est, errS, fixScale, x);
    int nBad = 0, nIn = 0;
    for (int stage = 0; stage < 2; stage++) {
        o.iters[stage] = levenberg_optimize(lm, stage == 0 ? 5 : (nBad > 0 ? 10 : 5), o.chi2[stage], o.lambda[stage]);
        o.stages = stage + 1;
        if (stage == 0) {
            nBad = ev.classify(errS, &nIn);
            o.nBad = nBad;
            if (n - nBad < 10) return;                               // :1211-1212: return 0, g2oS12 untouched
        } else ev.classify(errS, &nIn);
    }
    for (int k = 0; k < 4; k++) o.q[k] = est.q[k];                   // g2oS12 = vSim3_recov->estimate()
    for (int k = 0; k < 3; k++) o.t[k] = est.t[k];
    o.s = est.s; o.nIn = nIn;
}

// an item's outputs from o (sim3_opt.cpp)
void sim3opt_store(const ::sind_sim3opt_item& q, const Sim3OptOut& o, const uint8_t* removed);
// -> 0, or what is wrong with the item: 1 a negative n, 2 a NULL array, 3 an inv_sigma2 that is negative or not finite, 4 an input Sim3 that is not finite
int sim3opt_check(const ::sind_sim3opt_item& q);

// the plain sequential evaluator (the host library's)
struct Sim3OptSeq {
    int n; const float* x1; const float* x2; const float* o1; const float* o2; const float* is1; const float* is2; Sim3Cam K1, K2; float th2; bool fixScale; uint8_t* removed;
    void sums(const Sim3Q& est, bool full, double* S) {
        Sim3Q T[SIM3OPT_TRANSFORMS], Ti[SIM3OPT_TRANSFORMS];
        const int m = full ? SIM3OPT_TRANSFORMS : 1;
        for (int k = 0; k < m; k++) s3_perturbed(est, k, fixScale, T[k], Ti[k]);
        const double delta = s3_delta(th2);
        for (int k = 0; k < SIM3OPT_ENTRIES; k++) S[k] = 0.0;
        double c[SIM3OPT_ENTRIES];
        for (int i = 0; i < n; i++) {
            if (removed[i]) continue;                                // optimizer.removeEdge(e12), removeEdge(e21)
            for (int side = 0; side < 2; side++) {
                if (side == 0) s3_edge_contrib(T, K1, x2[3 * i], x2[3 * i + 1], x2[3 * i + 2], o1[2 * i], o1[2 * i + 1], is1[i], delta, full, c);
                else s3_edge_contrib(Ti, K2, x1[3 * i], x1[3 * i + 1], x1[3 * i + 2], o2[2 * i], o2[2 * i + 1], is2[i], delta, full, c);
                if (full) for (int k = 0; k < 35; k++) S[k] = S[k] + c[k];
                S[35] = S[35] + c[35];
            }
        }
    }
    int classify(const Sim3Q& Serr, int* nIn) {
        Sim3Q Sinv; s3_inverse(Serr, Sinv);
        int nBad = 0, in = 0;
        for (int i = 0; i < n; i++) {
            if (removed[i]) continue;                                // if(!e12 || !e21) continue;
            if (s3_pair_is_bad(Serr, Sinv, K1, K2, &x1[3 * i], &x2[3 * i], &o1[2 * i], &o2[2 * i], is1[i], is2[i], th2)) { removed[i] = 1; nBad++; } else in++;
        }
        *nIn = in;
        return nBad;
    }
};

}  // namespace sind
