// Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:781-1044; LoopClosing::CorrectLoop, src/LoopClosing.cc:567) written out without g2o: K key frames as
// VertexSim3Expmap (not marginalised, pLoopKF fixed), binary EdgeSim3 with the identity as information and no robust kernel, Levenberg-Marquardt with
// setUserLambdaInit(1e-16), optimize(20), then the pose recovery of every key frame and the correction of every map point through its reference key frame.  ONE source
// for the host (libsind_host.so: sindh_essential_graph, essential_graph.cpp) and the device (../match_essgraph.hip: k_ess_graph, k_ess_points): IEEE FP64 add / mul /
// div / sqrt on both sides, no contraction (-ffp-contract=off), every sum in a stated order, so the two give the same bits.  As in local_ba.hpp every phase is a
// function of ONE output element and the control flow (essential_graph<Ex>) is a template over an executor:
//   ex.par(n, f)   f(0) ... f(n - 1), each writing only its own outputs and reading nothing another element of the same phase writes.  Host: a plain loop.  Device:
//                  the lanes of one workgroup stride over the elements, then one barrier.
//   ex.rd(p), ex.rdi(p)   a scalar that a phase left in the workspace, read for the control flow (device: every lane reads it, then a barrier).
// The Levenberg-Marquardt scalars are computed by every lane from the same workspace values, so the control flow is uniform over the workgroup.
//
// RECALLED (not defined again): Sim3Q, s3_exp, s3_exp7, s3_mul, s3_inverse, s3_map, s3_oplus, s3_perturbed, s3_from_input (sim3_opt.hpp); po_sincos, po_quat_to_matrix
// (pose_opt.hpp); ba_chain (ba_schur.hpp); levenberg_optimize (g2o_lm.hpp), here with the user's initial lambda.
// DEFINED here: s3_log_d and s3_acos_d (std::log and acos), s3_lu3_solve, s3_log (Sim3::log), the phases ess_*, the envelope LDL^T, EssLm, essential_graph, ess_point.
//
// THE LITERAL READINGS of g2o.
// Vertices.  VertexSim3Expmap with _fix_scale; oplusImpl zeroes update[6] in the solver's own vector when it is set, then setEstimate(Sim3(update) * estimate()).  The
//   estimate starts as vScw[i]: the CorrectedSim3 entry if there is one, else Sim3(Rcw, tcw, 1.0) (s3_from_input; the quaternion is not normalised).  A free vertex with
//   at least one edge gets a Hessian index; sortVectorContainers orders the active vertices by id, key frames come in ascending mnId, so the indices ascend with the
//   key frame's position in the item.  A fixed vertex and a vertex without edges keep their estimate.
// Edges.  In the item's order (g2o's internal edge id is the insertion order).  Vertex 0 is edge_i, vertex 1 is edge_j.  The measurement is Sjw * Swi: for kind 0 (a
//   LoopConnections edge, :857-872) from vScw of both ends, for kind 1 (spanning tree, loop edges, covisibility, :889-979) from the NonCorrectedSim3 entry of an end
//   where there is one, else vScw.  computeError: _error = (C * v1->estimate() * v2->estimate().inverse()).log(), the products left to right.  chi2 = e . (I e): the
//   seven squares added in ascending order; activeChi2 is one chain over the edges in ascending order (ba_chain<8>).
// Sim3::log (sim3.h:148-230).  sigma = log(s); R = toRotationMatrix; d = 0.5 * (R00 + R11 + R22 - 1); the four branches on fabs(sigma) < eps and d > 1 - eps exactly
//   as written, with cos and sin of theta from po_sincos; W = (A Omega + B Omega2) + C I entry by entry as s3_exp7 has it, Omega2 = Omega * Omega; upsilon =
//   W.lu().solve(t), DEFINED as s3_lu3_solve: elimination with partial pivoting (the FIRST largest |entry| of the column from the diagonal down), the multipliers
//   f = a(r,c) / a(c,c), a(r,k) = a(r,k) - f * a(c,k), b(r) = b(r) - f * b(c), then back substitution ((b0 - a01 u1) - a02 u2) / a00.
// The Jacobians are NUMERIC: EdgeSim3 has no linearizeOplus, so BaseBinaryEdge::linearizeOplus runs (base_binary_edge.hpp:131-205): per free vertex and dimension d,
//   oplus(+1e-9 e_d), computeError, oplus(-1e-9 e_d), computeError, column d = (1 / 2e-9) * (e+ - e-).  A fixed vertex gets no Jacobian.  The 14 perturbed estimates of
//   a vertex (and their inverses, which is what vertex 1 enters the error with) do not depend on the edge: ess_perturb forms them once per vertex per linearisation with
//   s3_perturbed (same arithmetic, same bits as once per edge).  That leaves per edge the error itself and 28 evaluations: the elements of ess_errors.
// constructQuadraticForm (base_binary_edge.hpp:55-115), Omega = I: H_ii += A^T A, H_jj += B^T B, b_i += A^T (-e), b_j += B^T (-e), every product a sum over the seven
//   error rows in ascending order.  The off-diagonal block lives at (smaller index, larger index): A^T B, or (A^T B)^T = B^T A when vertex 0 has the larger index; the
//   two are each other's transposes bit for bit.  Each entry of a diagonal block and of b is a sequential sum from 0 over the vertex's edges in ascending edge order;
//   each entry of an off-diagonal block is a sequential sum from 0 over the edges of that pair of key frames in ascending edge order (several edges may join one pair:
//   LoopConnections holds both directions).  The lists are built by the host layer (EssPlan).  Only the upper triangle of a diagonal block is formed and mirrored; with
//   Omega = I both triangles are equal bit for bit anyway.
// The driver.  OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16): computeLambdaInit returns the user value when it is > 0.  optimize(20).  setLambda adds
//   lambda to every diagonal entry.  computeScale runs over x in index order.  x starts as zeros at buildStructure; a failed solve leaves it untouched.
// The linear solve.  The reference uses LinearSolverEigen: SimplicialLDLT under AMD ordering, which cannot be reproduced.  DEFINED, as in local_ba.hpp: the dense LDL^T
//   of H + lambda I (n = 7 * active vertices) in natural order without pivoting; entry (i, j), i >= j, is v = H(j,i); for k < j ascending: v = v - (L(i,k) * D(k)) *
//   L(j,k); D(j) = v at i = j, L(i,j) = v / D(j).  A zero pivot fails the solve and leaves x untouched; a NaN pivot does not fail (it poisons the trial's chi2).  The
//   solves: y(i) -= L(i,j) y(j) in ascending j, y(i) / D(i), y(i) -= L(j,i) y(j) in descending j.
//   STORED AND COMPUTED AS AN ENVELOPE (skyline).  first(I) is the first block column of block row I with a structural non-zero (an edge to a vertex of smaller index, or
//   I itself); every scalar row of block row I is stored from column 7 first(I) to its block's last column.  The k loop of entry (i, j) starts at max(fcol(i), fcol(j)),
//   fcol the row's first stored column.  Why that is the dense definition bit for bit, for finite values: by induction over k the dense L(i,k) with k < fcol(i) is an
//   exact zero (H(i,k) is a structural zero and every term of its sum has the factor L(i,k') = 0, k' < k; 0 / D(k) = 0), so each skipped term (L(i,k) * D(k)) * L(j,k)
//   is a product with an exact zero, +0 or -0, and v - (+-0) = v for every non-zero v.  The one exception is the sign of a zero: a chain value of -0 minus a skipped
//   -0 would be +0 in the dense form and stays -0 here; a -0 can only enter a chain as H(j,i) itself, which the ordered sums never produce from 0.0 + ..., and it
//   compares, multiplies and divides as +0 does in every later step but the sign of a quotient that is itself zero.  The same holds for the skipped terms of both
//   substitutions.  With an infinite or NaN D(k) the dense form would turn 0 * D into NaN where the envelope skips it: such a
//   factorisation is already poisoned, and its trial is rejected either way, but the bits of a NaN run are not claimed equal to the dense definition.
//   The cost follows the envelope: sum over the rows of (row length)^2 / 2 instead of n^3 / 6.
// Recovery (:999-1009).  Tiw = toCvSE3(q.toRotationMatrix(), t * (1. / s)) in float, for every key frame.  Points (:1020-1040): x3Dw_out = the float of
//   Siw_out[ref].inverse().map(vScw[ref].map(P)), P the double of the float input.
//
// UNPINNED PARITY (g2o and Eigen are not available to build or run; restated from the reference's Thirdparty/g2o and Eigen 3.3 as remembered).
//   1. everything sim3_opt.hpp and g2o_lm.hpp list (Eigen's evaluation order in the small products, -march=native contraction, po_sincos, s3_exp, x * x * x for pow).
//   2. the linear system: a natural-order envelope LDL^T here, SimplicialLDLT under AMD ordering there.
//   3. W.lu().solve(t): Eigen's PartialPivLU of a 3 x 3 (its blocked kernel's operation order) there, s3_lu3_solve here.
//   4. std::log and acos: the C library's there.  Here s3_log_d restates fdlibm's e_log.c (argument reduction by exact scaling, frexp, instead of the exponent field; the
//      three compares on the high word written as compares with the doubles those words denote) and s3_acos_d restates e_acos.c (the head of sqrt(z) taken by Dekker's
//      split with 2^27 + 1 instead of clearing the low word: it has at most 26 bits, so df * df is exact as the original's is).  log(1) = 0 and acos(1) = 0 exactly, NaN
//      outside the domain.
//   5. Eigen's order inside deltaR, skew and the trace; A^T Omega A with Omega = I is taken as A^T A (the products with 1 and the sums with 0 are exact).
//   6. the reference's iteration orders by pointer value (GetAllKeyFrames, LoopConnections and its sets, GetLoopEdges): whatever edge order the caller passes here.
// NOT OFFERED: a stop flag; global bundle adjustment.
// LIMITS (beyond them SIND_E_CAPACITY): ESS_MAX_KF key frames, ESS_MAX_EDGES edges, ESS_MAX_MP points, ESS_MAX_ENV stored entries of the factor's envelope.
#pragma once
#include <vector>
#include "sim3_opt.hpp"
#include "ba_schur.hpp"                                              // ba_chain

struct sind_essgraph_item;

namespace sind {

#define ESS_MAX_KF 4096
#define ESS_MAX_EDGES 65536
#define ESS_MAX_MP (1 << 20)
#define ESS_MAX_ENV (1 << 24)
#define ESS_NERR 29                                                  // error evaluations per edge: 0 the estimate; 1 + 2 d, 2 + 2 d vertex 0 after +-delta e_d; 15 + 2 d, 16 + 2 d vertex 1
#define ESS_C 119                                                    // doubles per edge: 0..27 A^T A (upper, row-major), 28..34 A^T (-e), 35..62 B^T B, 63..69 B^T (-e), 70..118 A^T B [7][7]
#define ESS_V 35                                                     // doubles per vertex: 28 of the diagonal block (upper, row-major), 7 of b
enum { ESS_SC_CHI = 0, ESS_SC_MAXD = 1, ESS_SC_SCALE = 2, ESS_SC_N = 8 };
enum { ESS_IS_FAIL = 0, ESS_IS_N = 8 };
struct EssDiag { double chi2, lambda; int iters, nActive, solverFail, pad; };

// One item as both executors see it: the caller's arrays digested by EssPlan (read only), the working state, the outputs.  All pointers are host or device alike.
struct EssView {
    int nKf, nE, nMp, nAct, nPair, n, fixScale;                      // n = 7 nAct
    const float* Tcw; const float* x3Dw;                             // [nKf][16], [nMp][3]
    const double* corr; const double* ncorr;                         // [nKf][8], [nKf][8]: qx qy qz qw tx ty tz s
    const int* hasC; const int* hasN; const int* mpRef;              // [nKf], [nKf], [nMp]
    const int* eI; const int* eJ; const int* eKind;                  // [nE]
    const int* vIdx; const int* idxV;                                // [nKf] Hessian index or -1; [nAct] its inverse
    const int* vEdgeStart; const int* vEdge;                         // [nAct + 1], [..] = 2 e + side (0: the vertex is vertex 0 of e), ascending e
    const int* pairStart; const int* pairLo; const int* pairHi; const int* pairE;   // [nPair + 1], [nPair] Hessian indices lo < hi, [..] = 2 e + (1: vertex 0 of e has index hi), ascending e
    const int* first; const int* rowOff; const int* blkLast;         // [nAct] first block column; [nAct] offset of the block row in M; [nAct] the last block row whose first <= this block column
    Sim3Q* vScw; Sim3Q* est; Sim3Q* bak; Sim3Q* meas; Sim3Q* Swc;    // [nKf], [nKf], [nKf], [nE], [nKf] = Siw_out.inverse()
    Sim3Q* T; Sim3Q* Ti;                                             // [nKf][15] the transforms of s3_perturbed and their inverses
    double* E; double* J; double* C; double* chiE;                   // [nE][29][7], [nE][2][7][7] (side, error row, dimension), [nE][ESS_C], [nE]
    double* Hd; double* Ho;                                          // [nAct][ESS_V], [nPair][49] the block (lo, hi), row-major
    double* M; double* Dg; double* y; double* x; double* term;       // the envelope: H + lambda I, then L; [n] each
    double* sc; int* isc;                                            // [ESS_SC_N], [ESS_IS_N]
    double* SiwOut; float* TiwOut; float* XOut; EssDiag* diag;       // [nKf][8], [nKf][16], [nMp][3], [1]
};

// ---------------------------------------------------------------- std::log, defined (see 4. above)
SIND_HD inline double s3_log_d(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, two20 = 1048576.0;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
    if (!(x == x)) return x;
    if (x < 0.0) return (x - x) / (x - x);                           // NaN
    if (x == 0.0) return -(DBL_MAX * 2.0);
    if (x > DBL_MAX) return x;
    int ex = 0;
    double xn = frexp(x, &ex) * 2.0;                                 // exact: x = xn 2^k, xn in [1, 2)
    int k = ex - 1;
    const bool halved = xn >= 1.0 + 434332.0 / two20;                // the high word's 0x6a09c: xn into [sqrt(2) / 2, sqrt(2))
    if (halved) { xn = xn * 0.5; k = k + 1; }
    const double f = xn - 1.0, dk = (double)k;
    if (f >= -1.0 / two20 && f < 1.0 / two20) {                      // |f| < 2^-20
        if (f == 0.0) { if (k == 0) return 0.0; return dk * ln2_hi + dk * ln2_lo; }
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        if (k == 0) return f - R;
        return dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6)), t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    const double R = t2 + t1;
    const bool mid = halved ? xn < (1.0 + 440402.0 / two20) * 0.5 : xn >= 1.0 + 398458.0 / two20;   // the high word in [0x6147a, 0x6b851]
    if (mid) {
        const double hfsq = 0.5 * f * f;
        if (k == 0) return f - (hfsq - s * (hfsq + R));
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    if (k == 0) return f - s * (f - R);
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}
// ---------------------------------------------------------------- acos, defined (see 4. above)
SIND_HD inline double s3_acos_d(double x) {
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01, pS3 = -4.00555345006794114027e-02,
                 pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
    const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01, qS4 = 7.70381505559019352791e-02;
    if (!(x == x)) return x;
    const double ax = fabs(x);
    if (ax >= 1.0) {
        if (ax == 1.0) return x > 0.0 ? 0.0 : pi + 2.0 * pio2_lo;
        return (x - x) / (x - x);                                    // NaN (inf - inf for an infinite x)
    }
    if (ax < 0.5) {
        if (ax <= 6.938893903907228e-18) return pio2_hi + pio2_lo;   // 2^-57
        const double z = x * x;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5))))), q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double r = p / q;
        return pio2_hi - (x - (pio2_lo - r * x));
    }
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5))))), q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double s = sqrt(z), r = p / q, w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5, s = sqrt(z);
    const double sp = s * 134217729.0, df = sp - (sp - s);           // the head of s: at most 26 bits
    const double c = (z - df * df) / (s + df);
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5))))), q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q, w = r * s + c;
    return 2.0 * (df + w);
}
// W.lu().solve(t), defined (see Sim3::log above)
SIND_HD inline void s3_lu3_solve(const double W[3][3], const double t[3], double u[3]) {
    double a[3][3], b[3];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) a[i][j] = W[i][j]; b[i] = t[i]; }
    for (int c = 0; c < 2; c++) {
        int piv = c; double best = fabs(a[c][c]);
        for (int r = c + 1; r < 3; r++) if (fabs(a[r][c]) > best) { best = fabs(a[r][c]); piv = r; }
        if (piv != c) { for (int k = 0; k < 3; k++) { const double s = a[c][k]; a[c][k] = a[piv][k]; a[piv][k] = s; } const double s = b[c]; b[c] = b[piv]; b[piv] = s; }
        for (int r = c + 1; r < 3; r++) {
            const double f = a[r][c] / a[c][c];
            for (int k = c + 1; k < 3; k++) a[r][k] = a[r][k] - f * a[c][k];
            b[r] = b[r] - f * b[c];
        }
    }
    u[2] = b[2] / a[2][2];
    u[1] = (b[1] - a[1][2] * u[2]) / a[1][1];
    u[0] = ((b[0] - a[0][1] * u[1]) - a[0][2] * u[2]) / a[0][0];
}
// Sim3::log (sim3.h:148-230)
SIND_HD inline void s3_log(const Sim3Q& S, double res[7]) {
    const double s = S.s, sigma = s3_log_d(s);
    double R[3][3]; po_quat_to_matrix(S.q, R);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};   // deltaR
    const double eps = 0.00001;
    double om[3], A, B, C;
    const bool nearI = d > 1 - eps;
    double theta = 0.0, sn = 0.0, cs = 1.0;
    if (nearI) { for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i]; }
    else {
        theta = s3_acos_d(d);
        const double f = theta / (2 * sqrt(1 - d * d));
        for (int i = 0; i < 3; i++) om[i] = f * dR[i];
        po_sincos(theta, &sn, &cs);
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (nearI) { A = 1. / 2.; B = 1. / 6.; }
        else { const double theta2 = theta * theta; A = (1 - cs) / (theta2); B = (theta - sn) / (theta2 * theta); }
    } else {
        C = (s - 1) / sigma;
        if (nearI) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta, a = s * sn, b = s * cs, c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const double O[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};   // skew
    double W[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
        const double o2 = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
        W[i][j] = (A * O[i][j] + B * o2) + C * (i == j ? 1.0 : 0.0);
    }
    double up[3]; s3_lu3_solve(W, S.t, up);
    for (int i = 0; i < 3; i++) { res[i] = om[i]; res[i + 3] = up[i]; }
    res[6] = sigma;
}
SIND_HD inline void s3_load8(const double* p, Sim3Q& S) { for (int k = 0; k < 4; k++) S.q[k] = p[k]; for (int k = 0; k < 3; k++) S.t[k] = p[4 + k]; S.s = p[7]; }
SIND_HD inline void s3_store8(const Sim3Q& S, double* p) { for (int k = 0; k < 4; k++) p[k] = S.q[k]; for (int k = 0; k < 3; k++) p[4 + k] = S.t[k]; p[7] = S.s; }
// EdgeSim3::computeError with the inverse of vertex 1's estimate given
SIND_HD inline void ess_edge_error(const Sim3Q& C, const Sim3Q& Si, const Sim3Q& SjInv, double e[7]) {
    Sim3Q a, b; s3_mul(C, Si, a); s3_mul(a, SjInv, b);
    s3_log(b, e);
}

// ---------------------------------------------------------------- the phases
// vScw and the starting estimates (:812-850), then the measurements (:857-979)
template <class Ex> SIND_HD inline void ess_init(Ex& ex, const EssView& w) {
    ex.par(w.nKf, [&](int i) {
        Sim3Q S;
        if (w.hasC[i]) s3_load8(&w.corr[8 * i], S);
        else {
            const float* T = &w.Tcw[16 * i];
            const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, t[3] = {T[3], T[7], T[11]};
            s3_from_input(1.0f, R, t, S);
        }
        w.vScw[i] = S; w.est[i] = S;
    });
    ex.par(w.nE, [&](int e) {
        const int i = w.eI[e], j = w.eJ[e];
        Sim3Q Siw = w.vScw[i], Sjw = w.vScw[j], Swi;
        if (w.eKind[e] == 1) { if (w.hasN[i]) s3_load8(&w.ncorr[8 * i], Siw); if (w.hasN[j]) s3_load8(&w.ncorr[8 * j], Sjw); }
        s3_inverse(Siw, Swi);
        s3_mul(Sjw, Swi, w.meas[e]);                                 // Sji = Sjw * Swi
        w.chiE[e] = 0.0;
    });
}
// the estimates as the edges read them: transform 0 (and its inverse) of every vertex; full: the 14 perturbed ones of every active vertex too
template <class Ex> SIND_HD inline void ess_perturb(Ex& ex, const EssView& w, bool full) {
    const int m = full ? SIM3OPT_TRANSFORMS : 1;
    ex.par(w.nKf * m, [&](int idx) {
        const int v = idx / m, k = idx % m;
        if (k > 0 && w.vIdx[v] < 0) return;
        s3_perturbed(w.est[v], k, w.fixScale != 0, w.T[v * SIM3OPT_TRANSFORMS + k], w.Ti[v * SIM3OPT_TRANSFORMS + k]);
    });
}
// computeError of every edge (and, full, of its 28 perturbations), chi2 of every edge
template <class Ex> SIND_HD inline void ess_errors(Ex& ex, const EssView& w, bool full) {
    const int m = full ? ESS_NERR : 1;
    ex.par(w.nE * m, [&](int idx) {
        const int e = idx / m, k = idx % m, i = w.eI[e], j = w.eJ[e];
        int ki = 0, kj = 0;
        if (k >= 15) { if (w.vIdx[j] < 0) return; kj = k - 14; }
        else if (k >= 1) { if (w.vIdx[i] < 0) return; ki = k; }
        double* out = &w.E[((size_t)e * ESS_NERR + k) * 7];
        ess_edge_error(w.meas[e], w.T[i * SIM3OPT_TRANSFORMS + ki], w.Ti[j * SIM3OPT_TRANSFORMS + kj], out);
        if (k == 0) { double c = 0.0; for (int d = 0; d < 7; d++) c = c + out[d] * out[d]; w.chiE[e] = c; }
    });
}
// the numeric Jacobians: J(side, row, d) = (1 / 2e-9) * (e+ - e-)
template <class Ex> SIND_HD inline void ess_jacobians(Ex& ex, const EssView& w) {
    ex.par(w.nE * 98, [&](int idx) {
        const int e = idx / 98, side = (idx % 98) / 49, row = (idx % 49) / 7, d = idx % 7;
        if (w.vIdx[side ? w.eJ[e] : w.eI[e]] < 0) return;
        const double scalar = 1.0 / (2 * 1e-9);
        const double* Ep = &w.E[((size_t)e * ESS_NERR + 1 + 14 * side + 2 * d) * 7];
        w.J[idx] = scalar * (Ep[row] - Ep[7 + row]);
    });
}
// constructQuadraticForm of every edge, one element per entry of ESS_C
template <class Ex> SIND_HD inline void ess_contrib(Ex& ex, const EssView& w) {
    ex.par(w.nE * ESS_C, [&](int idx) {
        const int e = idx / ESS_C, k = idx % ESS_C;
        const bool fi = w.vIdx[w.eI[e]] >= 0, fj = w.vIdx[w.eJ[e]] >= 0;
        const double* A = &w.J[(size_t)e * 98]; const double* B = A + 49; const double* er = &w.E[(size_t)e * ESS_NERR * 7];
        const double* L; const double* R; int r, c;
        if (k < 70) {
            const int side = k / 35, kk = k % 35;
            if (!(side ? fj : fi)) return;
            L = side ? B : A;
            if (kk >= 28) { r = kk - 28; double t = 0.0; for (int d = 0; d < 7; d++) t = t + L[7 * d + r] * -er[d]; w.C[idx] = t; return; }
            r = 0; c = kk; while (c >= 7 - r) { c -= 7 - r; r++; } c += r;           // entry kk of the upper triangle, row-major
            R = L;
        } else {
            if (!(fi && fj)) return;
            r = (k - 70) / 7; c = (k - 70) % 7; L = A; R = B;
        }
        double h = 0.0;
        for (int d = 0; d < 7; d++) h = h + L[7 * d + r] * R[7 * d + c];
        w.C[idx] = h;
    });
}
// the ordered sums of buildSystem (full) and activeChi2 -> sc[ESS_SC_CHI]
template <class Ex> SIND_HD inline void ess_sums(Ex& ex, const EssView& w, bool full) {
    const int nV = full ? w.nAct * ESS_V : 0, nP = full ? w.nPair * 49 : 0;
    ex.par(nV + nP + 1, [&](int idx) {
        double s = 0.0;
        if (idx < nV) {
            const int a = idx / ESS_V, k = idx % ESS_V;
            for (int q = w.vEdgeStart[a]; q < w.vEdgeStart[a + 1]; q++) { const int ce = w.vEdge[q]; s = s + w.C[(size_t)(ce >> 1) * ESS_C + 35 * (ce & 1) + k]; }
            w.Hd[idx] = s;
        } else if (idx < nV + nP) {
            const int p = (idx - nV) / 49, r = ((idx - nV) % 49) / 7, c = (idx - nV) % 7;
            for (int q = w.pairStart[p]; q < w.pairStart[p + 1]; q++) { const int ce = w.pairE[q]; s = s + w.C[(size_t)(ce >> 1) * ESS_C + 70 + ((ce & 1) ? 7 * c + r : 7 * r + c)]; }
            w.Ho[idx - nV] = s;
        } else w.sc[ESS_SC_CHI] = ba_chain<8>(w.chiE, w.nE);
    });
}
SIND_HD inline int ess_tri(int r, int c) { return r * 7 - r * (r - 1) / 2 + (c - r); }     // entry (r, c), r <= c, of a 7 x 7 upper triangle stored row-major
// the maxDiagonal of computeLambdaInit (not read when the user's lambda is > 0) -> sc[ESS_SC_MAXD]
template <class Ex> SIND_HD inline void ess_maxdiag(Ex& ex, const EssView& w) {
    ex.par(1, [&](int) {
        double maxDiagonal = 0.0;
        for (int a = 0; a < w.nAct; a++) for (int j = 0; j < 7; j++) { const double v = fabs(w.Hd[a * ESS_V + ess_tri(j, j)]); maxDiagonal = (v < maxDiagonal) ? maxDiagonal : v; }
        w.sc[ESS_SC_MAXD] = maxDiagonal;
    });
}
// the envelope: scalar row i = 7 I + r lies at M + rowOff[I] + r * 7 (I - first[I] + 1), its first stored column is 7 first[I]
SIND_HD inline double* ess_row(const EssView& w, int i, int& fcol) {
    const int I = i / 7; fcol = 7 * w.first[I];
    return w.M + w.rowOff[I] + (size_t)(i % 7) * (7 * (I - w.first[I] + 1)) - fcol;        // indexed by the column
}
// setLambda, the factorisation and both solves -> x; isc[ESS_IS_FAIL] != 0: a zero pivot, x untouched
template <class Ex> SIND_HD inline void ess_solve(Ex& ex, const EssView& w, double lambda) {
    const int n = w.n;
    ex.par(w.nAct * 7, [&](int i) {                                  // a row of zeros, then its diagonal block (lower part and diagonal) and b
        int fc; double* row = ess_row(w, i, fc);
        const int I = i / 7, r = i % 7;
        for (int c = fc; c < 7 * I; c++) row[c] = 0.0;
        for (int c = 0; c <= r; c++) { double v = w.Hd[I * ESS_V + ess_tri(c, r)]; if (c == r) v = v + lambda; row[7 * I + c] = v; }
        w.y[i] = w.Hd[I * ESS_V + 28 + r];
    });
    ex.par(w.nPair * 49, [&](int idx) {                              // the block (lo, hi) into the lower triangle at (hi, lo), transposed
        const int p = idx / 49, r = (idx % 49) / 7, c = idx % 7;
        int fc; double* row = ess_row(w, 7 * w.pairHi[p] + c, fc);
        row[7 * w.pairLo[p] + r] = w.Ho[idx];
    });
    for (int j = 0; j < n; j++) {                                    // LDL^T, column by column; every lane of the column forms D(j) for itself
        const int last = 7 * w.blkLast[j / 7] + 6;
        ex.par(last - j + 1, [&](int t) {
            const int i = j + t;
            int fi, fj; double* ri = ess_row(w, i, fi); const double* rj = ess_row(w, j, fj);
            if (fi > j) return;                                      // outside the envelope: a structural zero
            double d = rj[j], v = ri[j];
            const int ks = (i == j) ? j : (fi > fj ? fi : fj);       // below ks only the pivot's chain runs, from ks on both chains; the order of either is ascending k
            int k = fj;
            for (; k + 4 <= ks; k += 4) {                            // four loads ahead of the four steps of the chain, so that it waits for the adder and not for memory
                const double l0 = rj[k], l1 = rj[k + 1], l2 = rj[k + 2], l3 = rj[k + 3], d0 = w.Dg[k], d1 = w.Dg[k + 1], d2 = w.Dg[k + 2], d3 = w.Dg[k + 3];
                d = d - (l0 * d0) * l0; d = d - (l1 * d1) * l1; d = d - (l2 * d2) * l2; d = d - (l3 * d3) * l3;
            }
            for (; k < ks; k++) { const double ljk = rj[k]; d = d - (ljk * w.Dg[k]) * ljk; }
            for (; k + 4 <= j; k += 4) {
                const double l0 = rj[k], l1 = rj[k + 1], l2 = rj[k + 2], l3 = rj[k + 3], d0 = w.Dg[k], d1 = w.Dg[k + 1], d2 = w.Dg[k + 2], d3 = w.Dg[k + 3];
                const double a0 = ri[k], a1 = ri[k + 1], a2 = ri[k + 2], a3 = ri[k + 3];
                d = d - (l0 * d0) * l0; v = v - (a0 * d0) * l0; d = d - (l1 * d1) * l1; v = v - (a1 * d1) * l1;
                d = d - (l2 * d2) * l2; v = v - (a2 * d2) * l2; d = d - (l3 * d3) * l3; v = v - (a3 * d3) * l3;
            }
            for (; k < j; k++) { const double ljk = rj[k], dk = w.Dg[k]; d = d - (ljk * dk) * ljk; v = v - (ri[k] * dk) * ljk; }
            if (i == j) w.Dg[j] = d; else ri[j] = v / d;
        });
    }
    ex.par(1, [&](int) { int f = 0; for (int j = 0; j < n; j++) if (w.Dg[j] == 0.0) f = 1; w.isc[ESS_IS_FAIL] = f; });
    if (ex.rdi(&w.isc[ESS_IS_FAIL])) return;
    for (int j = 0; j < n; j++) {
        const int last = 7 * w.blkLast[j / 7] + 6;
        ex.par(last - j, [&](int t) { const int i = j + 1 + t; int fi; const double* ri = ess_row(w, i, fi); if (fi <= j) w.y[i] = w.y[i] - ri[j] * w.y[j]; });
    }
    ex.par(n, [&](int i) { w.y[i] = w.y[i] / w.Dg[i]; });
    for (int j = n - 1; j > 0; j--) {
        int fj; const double* rj = ess_row(w, j, fj);
        ex.par(j - fj, [&](int t) { const int i = fj + t; w.y[i] = w.y[i] - rj[i] * w.y[j]; });
    }
    ex.par(n, [&](int i) { w.x[i] = w.y[i]; });
}
// SparseOptimizer::update over the index mapping; oplusImpl zeroes x[6] of a vertex in place under fix_scale
template <class Ex> SIND_HD inline void ess_update(Ex& ex, const EssView& w) {
    ex.par(w.nAct, [&](int a) { s3_oplus(&w.x[7 * a], w.fixScale != 0, w.est[w.idxV[a]]); });
}
// computeScale (optimization_algorithm_levenberg.cpp:182-189) -> sc[ESS_SC_SCALE]
template <class Ex> SIND_HD inline void ess_scale(Ex& ex, const EssView& w, double lambda) {
    ex.par(w.n, [&](int i) { const double xj = w.x[i]; w.term[i] = xj * (lambda * xj + w.Hd[(i / 7) * ESS_V + 28 + i % 7]); });
    ex.par(1, [&](int) { w.sc[ESS_SC_SCALE] = ba_chain<8>(w.term, w.n); });
}

// optimize(20) as levenberg_optimize's problem
template <class Ex> struct EssLm {
    Ex& ex; const EssView& w; int fails;
    SIND_HD double linearize() { ess_perturb(ex, w, true); ess_errors(ex, w, true); ess_jacobians(ex, w); ess_contrib(ex, w); ess_sums(ex, w, true); return ex.rd(&w.sc[ESS_SC_CHI]); }
    SIND_HD double max_diagonal() { ess_maxdiag(ex, w); return ex.rd(&w.sc[ESS_SC_MAXD]); }
    SIND_HD void push() { ex.par(w.nKf, [&](int i) { w.bak[i] = w.est[i]; }); }
    SIND_HD bool solve(double lambda) { ess_solve(ex, w, lambda); const bool ok = ex.rdi(&w.isc[ESS_IS_FAIL]) == 0; if (!ok) fails++; return ok; }
    SIND_HD void update() { ess_update(ex, w); }
    SIND_HD double chi2() { ess_perturb(ex, w, false); ess_errors(ex, w, false); ess_sums(ex, w, false); return ex.rd(&w.sc[ESS_SC_CHI]); }
    SIND_HD double scale(double lambda) { ess_scale(ex, w, lambda); return ex.rd(&w.sc[ESS_SC_SCALE]); }
    SIND_HD void pop() { ex.par(w.nKf, [&](int i) { w.est[i] = w.bak[i]; }); }
};

// the graph part of the function: everything but the points
template <class Ex> SIND_HD inline void essential_graph(Ex& ex, const EssView& w) {
    ess_init(ex, w);
    EssDiag dg; dg.chi2 = 0.0; dg.lambda = -1.0; dg.iters = -1; dg.nActive = w.nAct; dg.solverFail = 0; dg.pad = 0;
    if (w.nAct > 0) {                                                // else: "0 vertices to optimize", optimize returns -1
        ex.par(w.n, [&](int i) { w.x[i] = 0.0; });                   // buildStructure
        EssLm<Ex> lm{ex, w, 0};
        dg.iters = levenberg_optimize(lm, 20, dg.chi2, dg.lambda, 1e-16);
        dg.solverFail = lm.fails;
    }
    ex.par(w.nKf + 1, [&](int i) {                                   // :999-1009
        if (i == w.nKf) { *w.diag = dg; return; }
        const Sim3Q S = w.est[i];
        s3_store8(S, &w.SiwOut[8 * i]);
        s3_inverse(S, w.Swc[i]);                                     // vCorrectedSwc[nIDi] = CorrectedSiw.inverse()
        double R[3][3]; po_quat_to_matrix(S.q, R);
        const double f = 1. / S.s;
        float* T = &w.TiwOut[16 * i];
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[r][c]; T[4 * r + 3] = (float)(S.t[r] * f); }
        T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
    });
}
// one map point (:1020-1040), after essential_graph
SIND_HD inline void ess_point(const EssView& w, int j) {
    const int r = w.mpRef[j];
    const double P[3] = {(double)w.x3Dw[3 * j], (double)w.x3Dw[3 * j + 1], (double)w.x3Dw[3 * j + 2]};
    double a[3], b[3];
    s3_map(w.vScw[r], P, a); s3_map(w.Swc[r], a, b);
    for (int k = 0; k < 3; k++) w.XOut[3 * j + k] = (float)b[k];
}

// ---------------------------------------------------------------- the host layer both entry points share (essential_graph.cpp)
// An item digested: the lists of EssView and the sizes of its working state.  I: every int array, the inputs and lists first, then the work ints (oIsc).
struct EssPlan {
    int nKf = 0, nE = 0, nMp = 0, nAct = 0, nPair = 0; size_t nEnv = 0;
    std::vector<int> I;
    size_t oHasC, oHasN, oMpRef, oEI, oEJ, oEKind, oVIdx, oIdxV, oVEdgeStart, oVEdge, oPairStart, oPairLo, oPairHi, oPairE, oFirst, oRowOff, oBlkLast, oIsc;
    ItemSizes z;                                                     // no ints come back; doubles in: corr, ncorr; the head: EssDiag, SiwOut
};
// -> 0, or what is wrong with the item (ess_check_text)
int ess_check(const ::sind_essgraph_item& q);
extern const char* const ess_check_text[];
// -> SIND_OK or SIND_E_CAPACITY; the item has passed ess_check
int ess_plan(const ::sind_essgraph_item& q, EssPlan& pl);
// the view of an item over its share of the streams (Fin: Tcw, x3Dw; Din: corr, ncorr, both filled by ess_fill; Fout: TiwOut, XOut; the head: EssDiag, SiwOut)
void ess_fill(const ::sind_essgraph_item& q, const ItemPtrs& p);
void ess_bind(const EssPlan& pl, int fixScale, const ItemPtrs& p, EssView& v);
// an item's outputs from what came back (p: host storage)
void ess_store(const ::sind_essgraph_item& q, const EssPlan& pl, const ItemPtrs& p);

}  // namespace sind
