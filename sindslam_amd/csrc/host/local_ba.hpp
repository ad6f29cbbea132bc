// Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:506-778) written out without g2o: P free 6-DoF poses, fixed poses, M marginalised points, binary
// reprojection edges (mono or stereo), Levenberg-Marquardt over the Schur complement of the points, optimize(5) with Huber kernels, the outliers moved to level 1,
// optimize(10) without kernels, the final classification.  ONE source for the host (libsind_host.so: sindh_local_ba, local_ba.cpp) and the device
// (../match_localba.hip: k_local_ba): IEEE FP64 add / mul / div / sqrt on both sides, no contraction (-ffp-contract=off), every sum in a stated order, so the two
// give the same bits.  The control flow (local_ba<Ex>) is a template over an executor.  Every phase of the algorithm (evaluate the edges, the ordered sums, Schur,
// LDLT and solve, back-substitution, update, classify) is written here ONCE as a function of one output element; the executor only says who runs the elements:
//   ex.par(n, f)   f(0) ... f(n - 1), each writing only its own outputs and reading nothing another element of the same phase writes.  Host: a plain loop.  Device:
//                  the lanes of one workgroup stride over the elements, then one barrier.
//   ex.rd(p)       a scalar that a phase left in the workspace, read for the control flow (device: every lane reads it, then a barrier, so the next phase may rewrite it).
// The Levenberg-Marquardt scalars are computed by every lane from the same workspace values, so the control flow is uniform over the workgroup.
//
// RECALLED from pose_opt.hpp (not defined again): PoseQ, po_from_tcw, po_to_tcw, po_quat_to_matrix, po_map, po_exp, po_mul, po_oplus, po_edge_error (the error and chi2
// of both edge types; the stereo cam_project keeps `const float invz`), po_huber, po_delta; from g2o_lm.hpp jtwj_upper and levenberg_optimize, the control flow of
// OptimizationAlgorithmLevenberg::solve with the literal points all three optimizers share.
// DEFINED here: lba_inv3, lba_edge (the two binary edges' linearizeOplus and constructQuadraticForm), the phases lba_*, their grouping into the driver's operations
// (LbaLm) and local_ba.
//
// THE CONTRACT that makes host and device equal, and what it restates of g2o.
// Vertex order (sparse_optimizer.cpp buildIndexMapping :166-190 over the sorted active vertices).  Poses first, then points, each in ascending id, over the vertices
//   active at the level.  Poses are ordered by kf_id.  Points are ordered by mp_id (point ids are all shifted by the same maxKFid+1, so the order is that of mnId).  A
//   vertex with no level-0 edge left in stage 2 is not active (initializeOptimization :206-267: _activeVertices holds a vertex only if it has at least one edge of the
//   requested level): it keeps its estimate, and the Hessian indices of the others close up.  A fixed key frame has no index; its edges contribute to the point side only.
// Edge order.  The item's observation order (g2o's internal edge id is the insertion order); mono and stereo edges interleaved as they were inserted.
// buildSystem (block_solver.hpp:502-560; base_binary_edge.hpp:55-115).  Hpp(i,i) and b_i of a pose, Hll(j,j) and b_j of a point are each a sequential FP64 sum from 0
//   over that vertex's active edges in ascending edge order.  Hpl(i,j) has exactly one contributing edge.  activeRobustChi2 is one sequential sum over all active edges
//   in ascending edge order.  The small products take every sum in ascending index order; Omega = invSigma2 * I is applied as one multiplication, as in po_edge_contrib:
//   H(i,j) = sum_d (J[d][i] * W) * J'[d][j] with W = rho1 * invSigma2 (W = invSigma2 without a kernel), for A^T W A, B^T W B and B^T W A alike (A: point, B: pose);
//   b += sum_d J[d][j] * wr[d] with wr = -(invSigma2 * e), times rho1 with a kernel.  Only the upper triangles of Hpp(i,i) and Hll(j,j) are formed and mirrored.
// setLambda (:564-589).  Lambda is added to every diagonal entry of Hpp and Hll.  computeLambdaInit is tau (1e-5) times the largest |diagonal| over all active poses
//   and points, one chain in vertex order with std::max's compare (a NaN diagonal wins).  computeScale runs over the whole of x, poses then points.
// Schur complement, with the loop nest and signs of block_solver.hpp:381-439.  Points are visited in ascending Hessian index.  Dinv = D.inverse() is Eigen's closed-form
//   3 x 3 inverse, DEFINED as lba_inv3: cyclic cofactors over the determinant (det = c00 m00 + c10 m10 + c20 m20).  db = Dinv * b_l.  The point's pose blocks are visited in
//   ascending row i1.  BDinv = Bi * Dinv, formed once per (point, pose).  coefficients_i1 += Bi * db.  For i2 >= i1: Hschur(i1,i2) -= BDinv * Bj^T; only the upper
//   triangle is formed (of a diagonal block too).  Then bschur = b_p - coefficients.  EVERY ENTRY of Hschur and coefficients therefore receives its contributions in
//   ascending point order: one element per entry walks the points both poses see in that order, over lists the host layer builds (LbaPlan).  Hschur starts as Hpp (with
//   lambda) on the diagonal blocks and 0 elsewhere.
// Reduced system.  The reference uses LinearSolverEigen: Eigen's SimplicialLDLT<Upper> under a scalar AMD ordering, which cannot be reproduced here.  DEFINED instead: a
//   dense LDL^T of the 6P x 6P matrix in natural order without pivoting; entry (i,j), i >= j, is one function of the finished columns,
//   v = H(j,i); for k < j ascending: v = v - (L(i,k) * D(k)) * L(j,k); D(j) = v at i = j, L(i,j) = v / D(j).  It fails when a pivot equals 0 (SimplicialLDLT's
//   NumericalIssue); x is then untouched.  A NaN pivot does not fail: it poisons tempChi and the step is rejected by g2o_isfinite.  The solves: y(i) -= L(i,j) y(j) in ascending
//   j, y(i) / D(i), y(i) -= L(j,i) y(j) in descending j.  With P = 0 (every pose fixed) the empty factorisation succeeds.
// Back-substitution (:461-481).  cl = bl - sum_i Hpl(i,j)^T xp_i in ascending pose row, as rightMultiply does it (cl += Hpl^T * (-xp)); xl = 0 + Dinv * cl.
// Update, push and pop.  po_oplus for poses, += for points; push and pop cover all active vertices.  Kept literally: after a rejected last trial the edges hold the
//   errors of the REJECTED state; the classification reads those, while isDepthPositive reads the restored estimates.  An edge at level 1 keeps the error of its last
//   evaluation in stage 1, and the final classification reads that.
// x starts as zeros at each buildStructure, that is at iteration 0 of each optimize call (the reference leaves it uninitialised).
// The function.  Stage 1: optimize(5), Huber on every edge, deltas the floats sqrt(5.991) and sqrt(7.815).  Classification: chi2() > 5.991 (mono) or > 7.815 (stereo) or
//   !isDepthPositive() -> level 1; the compares are in double (not in float as in PoseOptimization); a NaN chi2 compares false, a NaN depth is not positive.  Kernels
//   removed from all edges.  Stage 2: initializeOptimization(0), optimize(10); an optimize with no active vertex does nothing (g2o returns -1) and is not counted in
//   n_stages.  The final classification gives vToErase.  Local key frames (kind 0 and 1) get toCvMat(estimate), a round trip through the quaternion; fixed cameras
//   (kind 2) are not written (their output rows are the input); points get the float of the estimate.  do_more = 0 is bDoMore = false: the stop flag seen after stage 1;
//   the level changes and stage 2 are then skipped.
// NOT OFFERED: a stop flag that flips in the middle of an optimize (terminate() is always false here).  pMP->isBad() during the call cannot happen: the item is a copy.
//
// UNPINNED PARITY (g2o and Eigen are not available to build or run; restated from the reference's Thirdparty/g2o and Eigen 3.3 as remembered).
//   1. everything pose_opt.hpp lists (Eigen's evaluation order in the small products, -march=native contraction, po_sincos, x * x * x for pow).
//   2. the reduced system: dense natural-order LDL^T here, SimplicialLDLT under AMD ordering there.
//   3. Eigen's order inside -1./z * tmp * R (here ((-1/z) tmp) R, three terms each, zeros included), inside Dinv * b, Bi * Dinv, Bi * db, BDinv * Bj^T and the 3 x 3 inverse.
//   4. the order of a point's observations: a std::map keyed by pointers there, whatever the caller passes here.
//   5. Hpp(i,i) and Hll(j,j) are accumulated full there (both triangles, which may differ in the last bit); the upper triangle mirrored here.
// LIMITS (beyond them SIND_E_CAPACITY): LBA_MAX_POSES free poses, LBA_MAX_KF key frames, LBA_MAX_MP points, LBA_MAX_OBS observations, LBA_MAX_PAIRS entries of the
// co-observation lists (sum over the points of k (k + 1) / 2, k = the point's observations in free poses).
#pragma once
#include <vector>
#include "pose_opt.hpp"

struct sind_localba_item;

namespace sind {

#define LBA_MAX_POSES 256
#define LBA_MAX_KF 4096
#define LBA_MAX_MP 65536
#define LBA_MAX_OBS (1 << 20)
#define LBA_MAX_PAIRS (1 << 24)
#define LBA_C 56                                                     // doubles per edge: 0..20 pose H (upper, row-major), 21..26 pose b, 27..32 point H (upper), 33..35 point b, 36..53 Hpl [6][3], 54 rho[0], 55 chi2()
enum { LBA_SC_CHI = 0, LBA_SC_MAXD = 1, LBA_SC_SCALE = 2, LBA_SC_N = 8 };
enum { LBA_IS_NP = 0, LBA_IS_NM = 1, LBA_IS_FAIL = 2, LBA_IS_NL1 = 3, LBA_IS_N = 8 };
struct LbaDiag { double chi2[2], lambda[2]; int stages, iters[2], nLevel1; };

// One item as both executors see it: the caller's arrays digested by LbaPlan (read only), the working state, the outputs.  All pointers are host or device alike.
struct LbaView {
    int nKf, nMp, nObs, P, nPair, doMore; PoseOptCam K;
    const float* Tcw; const float* x3Dw; const float* eObs;         // [nKf][16], [nMp][3], [nObs][4] = x y uRight invSigma2
    const int* kfKind; const int* kfPose; const int* poseKf;         // [nKf] the item's kind; [nKf] rank of a kind-0 key frame by kf_id, else -1; [P] its inverse
    const int* ptOrder; const int* obsStart;                         // [nMp] the points in ascending mp_id; [nMp + 1]
    const int* ePt; const int* eKf;                                  // [nObs]
    const int* poseEdgeStart; const int* poseEdge;                   // [P + 1], [..]: the edges of a free pose in ascending edge order
    const int* ptNF; const int* ptSorted;                            // [nMp], [nObs]: at obsStart[j], ptNF[j] edges of point j into free poses, in ascending pose rank
    const int* pairStart; const int* pairKey; const int* pairE;      // [nPair + 1], [nPair] = s1 * LBA_MAX_POSES + s2 (s1 <= s2), [..][2] = (edge into s1, edge into s2) in ascending point order
    const int* diagPair;                                             // [P] the pair (s, s), -1 without an edge
    PoseQ* est; PoseQ* bak; double* X; double* Xbak;                 // [nKf], [nKf], [nMp][3], [nMp][3]
    double* C; double* BD;                                           // [nObs][LBA_C], [nObs][18] BDinv
    double* Hpp; double* Hll; double* Dinv; double* db;              // [P][27] = 21 + 6, [nMp][9] = 6 + 3, [nMp][9], [nMp][3]
    double* Hs; double* Lm; double* Dg; double* y;                   // [n][n] row-major (upper), [n][n] L(i,k) at k * n + i, [n], [n]; n = 6 * active poses <= 6 P
    double* x; double* sc;                                           // [6 P + 3 nMp] by pose rank and item point, [LBA_SC_N]
    double* rho; double* term;                                       // [nObs] rho[0] of an edge, 0 at level 1; [6 P + 3 nMp] the terms of computeScale in vertex order, 0 for an inactive vertex
    int* level; int* poseIdx; int* ptAct; int* isc;                  // [nObs], [P] Hessian index or -1, [nMp], [LBA_IS_N]
    float* TcwOut; float* XOut; int* erase; LbaDiag* diag;           // [nKf][16], [nMp][3], [nObs], [1]
};

// Eigen's closed-form inverse of a 3 x 3 (Eigen/src/LU/InverseImpl.h: compute_inverse<.., 3>, cofactor_3x3): inv(i,j) = cofactor(j,i) * (1 / det)
SIND_HD inline double lba_cof(const double m[3][3], int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
}
SIND_HD inline void lba_inv3(const double m[3][3], double inv[3][3]) {
    const double c0 = lba_cof(m, 0, 0), c1 = lba_cof(m, 1, 0), c2 = lba_cof(m, 2, 0);
    const double det = c0 * m[0][0] + c1 * m[1][0] + c2 * m[2][0];
    const double invdet = 1.0 / det;
    inv[0][0] = c0 * invdet; inv[0][1] = c1 * invdet; inv[0][2] = c2 * invdet;
    for (int i = 1; i < 3; i++) for (int j = 0; j < 3; j++) inv[i][j] = lba_cof(m, j, i) * invdet;
}

// One edge: computeError (+ robustify); full: linearizeOplus (types_six_dof_expmap.cpp:103-139, :188-234, as written: divisions by z and z_2) and
// constructQuadraticForm.  poseFree: vertex 1 is not fixed.  c: see LBA_C; not full: c[54] and c[55] alone; !poseFree: the pose entries and Hpl stay unwritten.
// jac (the tests'): _jacobianOplusXi [3][3], _jacobianOplusXj [3][6] and the error [3].  delta: the Huber deltas [mono, stereo] of a caller whose are not po_delta's
// (global_ba.hpp: Optimizer::BundleAdjustment's sqrt(5.99)); NULL: po_delta, local BA's
SIND_HD inline void lba_edge(const PoseQ& P, const PoseOptCam& K, const double X[3], const float* ob, bool robust, bool full, bool poseFree, double* c, double* jac = nullptr, const double* delta = nullptr) {
    const bool stereo = !(ob[2] < 0.0f);                             // if(pKFi->mvuRight[mit->second]<0) mono (Optimizer.cc:594)
    const double s = (double)ob[3];
    double e[3], Xc[3];
    const double chi2 = po_edge_error(P, K, X, (double)ob[0], (double)ob[1], (double)ob[2], stereo, s, e, Xc);
    double rho0 = chi2, rho1 = 1.0;
    if (robust) po_huber(chi2, delta ? delta[stereo ? 1 : 0] : po_delta(stereo), &rho0, &rho1);
    c[54] = rho0; c[55] = chi2;
    if (!full) return;
    double R[3][3]; po_quat_to_matrix(P.q, R);
    const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z, fx = K.fx, fy = K.fy, bf = K.bf;
    double A[3][3], B[3][6];
    if (!stereo) {
        const double tmp[2][3] = {{fx, 0.0, -x / z * fx}, {0.0, fy, -y / z * fy}};
        const double m = -1. / z;                                    // _jacobianOplusXi = -1./z * tmp * T.rotation().toRotationMatrix()
        for (int r = 0; r < 2; r++) for (int q = 0; q < 3; q++) A[r][q] = (m * tmp[r][0]) * R[0][q] + (m * tmp[r][1]) * R[1][q] + (m * tmp[r][2]) * R[2][q];
        for (int q = 0; q < 3; q++) A[2][q] = 0.0;
    } else {
        for (int q = 0; q < 3; q++) {
            A[0][q] = -fx * R[0][q] / z + fx * x * R[2][q] / z_2;
            A[1][q] = -fy * R[1][q] / z + fy * y * R[2][q] / z_2;
            A[2][q] = A[0][q] - bf * R[2][q] / z_2;
        }
    }
    B[0][0] = x * y / z_2 * fx; B[0][1] = -(1 + (x * x / z_2)) * fx; B[0][2] = y / z * fx; B[0][3] = -1. / z * fx; B[0][4] = 0; B[0][5] = x / z_2 * fx;
    B[1][0] = (1 + y * y / z_2) * fy; B[1][1] = -x * y / z_2 * fy; B[1][2] = -x / z * fy; B[1][3] = 0; B[1][4] = -1. / z * fy; B[1][5] = y / z_2 * fy;
    if (stereo) {
        B[2][0] = B[0][0] - bf * y / z_2; B[2][1] = B[0][1] + bf * x / z_2; B[2][2] = B[0][2]; B[2][3] = B[0][3]; B[2][4] = 0; B[2][5] = B[0][5] - bf / z_2;
    } else { for (int j = 0; j < 6; j++) B[2][j] = 0.0; }
    if (jac) { for (int d = 0; d < 3; d++) { for (int q = 0; q < 3; q++) jac[3 * d + q] = A[d][q]; for (int q = 0; q < 6; q++) jac[9 + 6 * d + q] = B[d][q]; jac[27 + d] = e[d]; } }
    const double W = robust ? rho1 * s : s;                          // weightedOmega = rho[1] * information
    double wr[3];                                                    // omega_r = - omega * _error; omega_r *= rho[1]
    for (int d = 0; d < 3; d++) { wr[d] = -(s * e[d]); if (robust) wr[d] = wr[d] * rho1; }
    jtwj_upper(A, W, stereo, c + 27);
    for (int j = 0; j < 3; j++) {
        double t = A[0][j] * wr[0] + A[1][j] * wr[1];
        if (stereo) t = t + A[2][j] * wr[2];
        c[33 + j] = t;
    }
    if (!poseFree) return;
    jtwj_upper(B, W, stereo, c);
    for (int j = 0; j < 6; j++) {
        double t = B[0][j] * wr[0] + B[1][j] * wr[1];
        if (stereo) t = t + B[2][j] * wr[2];
        c[21 + j] = t;
    }
    for (int r = 0; r < 6; r++) for (int q = 0; q < 3; q++) {
        double h = (B[0][r] * W) * A[0][q] + (B[1][r] * W) * A[1][q];
        if (stereo) h = h + (B[2][r] * W) * A[2][q];
        c[36 + 3 * r + q] = h;
    }
}

// ---------------------------------------------------------------- the phases
// a[0] + a[1] + ... in that order from 0, one lane.  The values lie densely so that the loads do not wait for the additions; an entry that g2o would not add (an edge
// at level 1, an inactive vertex) holds +0.0, and s + 0.0 == s for every s such a sum can hold: it starts as +0.0 and a sum is -0.0 only if both operands are
SIND_HD inline double lba_chain(const double* a, int n) {
    double s = 0.0; int i = 0;
    for (; i + 8 <= n; i += 8) {
        const double v0 = a[i], v1 = a[i + 1], v2 = a[i + 2], v3 = a[i + 3], v4 = a[i + 4], v5 = a[i + 5], v6 = a[i + 6], v7 = a[i + 7];
        s = s + v0; s = s + v1; s = s + v2; s = s + v3; s = s + v4; s = s + v5; s = s + v6; s = s + v7;
    }
    for (; i < n; i++) s = s + a[i];
    return s;
}
// the same over entry k of the edges of a list (Ck = C + k): four edges' indices, levels and values are fetched before the four additions
SIND_HD inline double lba_chain_edges(const int* list, int n, const int* level, const double* Ck) {
    double s = 0.0; int a = 0;
    for (; a + 4 <= n; a += 4) {
        const int e0 = list[a], e1 = list[a + 1], e2 = list[a + 2], e3 = list[a + 3];
        const int l0 = level[e0], l1 = level[e1], l2 = level[e2], l3 = level[e3];
        const double v0 = Ck[(size_t)e0 * LBA_C], v1 = Ck[(size_t)e1 * LBA_C], v2 = Ck[(size_t)e2 * LBA_C], v3 = Ck[(size_t)e3 * LBA_C];
        s = s + (l0 ? 0.0 : v0); s = s + (l1 ? 0.0 : v1); s = s + (l2 ? 0.0 : v2); s = s + (l3 ? 0.0 : v3);
    }
    for (; a < n; a++) { const int e = list[a]; s = s + (level[e] ? 0.0 : Ck[(size_t)e * LBA_C]); }
    return s;
}
// computeActiveErrors (+ linearizeOplus + constructQuadraticForm if full) over the level-0 edges
template <class Ex> SIND_HD inline void lba_eval(Ex& ex, const LbaView& w, bool robust, bool full) {
    ex.par(w.nObs, [&](int e) {
        if (w.level[e]) { w.rho[e] = 0.0; return; }
        const int kf = w.eKf[e];
        lba_edge(w.est[kf], w.K, &w.X[3 * w.ePt[e]], &w.eObs[4 * e], robust, full, w.kfPose[kf] >= 0, &w.C[(size_t)e * LBA_C]);
        w.rho[e] = w.C[(size_t)e * LBA_C + 54];
    });
}
// the ordered sums of buildSystem (full) and activeRobustChi2 -> sc[LBA_SC_CHI]
template <class Ex> SIND_HD inline void lba_sums(Ex& ex, const LbaView& w, bool full) {
    const int nP = full ? w.P * 27 : 0, nM = full ? w.nMp * 9 : 0;
    ex.par(nP + nM + 1, [&](int idx) {
        double s = 0.0;
        if (idx < nP) {
            const int p = idx / 27, k = idx % 27;
            w.Hpp[idx] = lba_chain_edges(w.poseEdge + w.poseEdgeStart[p], w.poseEdgeStart[p + 1] - w.poseEdgeStart[p], w.level, w.C + k);
        } else if (idx < nP + nM) {
            const int j = (idx - nP) / 9, k = (idx - nP) % 9;
            for (int e = w.obsStart[j]; e < w.obsStart[j + 1]; e++) if (!w.level[e]) s = s + w.C[(size_t)e * LBA_C + 27 + k];
            w.Hll[idx - nP] = s;
        } else {
            w.sc[LBA_SC_CHI] = lba_chain(w.rho, w.nObs);
        }
    });
}
// initializeOptimization(0) + buildIndexMapping: which vertices are active, the Hessian indices of the poses -> isc[LBA_IS_NP], isc[LBA_IS_NM]
template <class Ex> SIND_HD inline void lba_activate(Ex& ex, const LbaView& w) {
    ex.par(w.P + w.nMp, [&](int idx) {
        int act = 0;
        if (idx < w.P) { for (int a = w.poseEdgeStart[idx]; a < w.poseEdgeStart[idx + 1]; a++) if (!w.level[w.poseEdge[a]]) act = 1; w.poseIdx[idx] = act; }
        else { const int j = idx - w.P; for (int e = w.obsStart[j]; e < w.obsStart[j + 1]; e++) if (!w.level[e]) act = 1; w.ptAct[j] = act; }
    });
    ex.par(1, [&](int) {
        int k = 0, m = 0;
        for (int p = 0; p < w.P; p++) w.poseIdx[p] = w.poseIdx[p] ? k++ : -1;
        for (int j = 0; j < w.nMp; j++) m += w.ptAct[j];
        w.isc[LBA_IS_NP] = k; w.isc[LBA_IS_NM] = m;
    });
}
// the maxDiagonal of computeLambdaInit -> sc[LBA_SC_MAXD]
template <class Ex> SIND_HD inline void lba_maxdiag(Ex& ex, const LbaView& w) {
    ex.par(1, [&](int) {
        double maxDiagonal = 0.0;
        const int dp[6] = {0, 6, 11, 15, 18, 20}, dl[3] = {0, 3, 5};
        for (int p = 0; p < w.P; p++) if (w.poseIdx[p] >= 0) for (int j = 0; j < 6; j++) { const double a = fabs(w.Hpp[p * 27 + dp[j]]); maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a; }
        for (int o = 0; o < w.nMp; o++) { const int q = w.ptOrder[o]; if (w.ptAct[q]) for (int j = 0; j < 3; j++) { const double a = fabs(w.Hll[q * 9 + dl[j]]); maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a; } }
        w.sc[LBA_SC_MAXD] = maxDiagonal;
    });
}
// push / pop over the vertices
template <class Ex> SIND_HD inline void lba_push(Ex& ex, const LbaView& w) {
    ex.par(w.nKf + w.nMp, [&](int i) { if (i < w.nKf) w.bak[i] = w.est[i]; else for (int k = 0; k < 3; k++) w.Xbak[3 * (i - w.nKf) + k] = w.X[3 * (i - w.nKf) + k]; });
}
template <class Ex> SIND_HD inline void lba_pop(Ex& ex, const LbaView& w) {
    ex.par(w.nKf + w.nMp, [&](int i) { if (i < w.nKf) w.est[i] = w.bak[i]; else for (int k = 0; k < 3; k++) w.X[3 * (i - w.nKf) + k] = w.Xbak[3 * (i - w.nKf) + k]; });
}
// BlockSolver::solve with setLambda(lambda): Schur complement, LDL^T, the two solves, back-substitution -> x; isc[LBA_IS_FAIL] != 0: a zero pivot, x untouched
template <class Ex> SIND_HD inline void lba_solve(Ex& ex, const LbaView& w, double lambda, int nAct) {
    const int n = 6 * nAct;
    ex.par(w.nMp + n * n, [&](int idx) {                             // Dinv and db of every active point; Hschur = 0
        if (idx >= w.nMp) { w.Hs[idx - w.nMp] = 0.0; return; }
        const int j = idx; if (!w.ptAct[j]) return;
        const double* h = &w.Hll[j * 9];
        const double D[3][3] = {{h[0] + lambda, h[1], h[2]}, {h[1], h[3] + lambda, h[4]}, {h[2], h[4], h[5] + lambda}};
        double inv[3][3]; lba_inv3(D, inv);
        for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) w.Dinv[j * 9 + 3 * r + q] = inv[r][q]; w.db[3 * j + r] = inv[r][0] * h[6] + inv[r][1] * h[7] + inv[r][2] * h[8]; }
    });
    ex.par(w.nObs, [&](int e) {                                      // BDinv = Bi * Dinv, once per (point, pose)
        if (w.level[e] || w.kfPose[w.eKf[e]] < 0) return;
        const double* Bi = &w.C[(size_t)e * LBA_C + 36]; const double* Di = &w.Dinv[w.ePt[e] * 9];
        for (int r = 0; r < 6; r++) for (int q = 0; q < 3; q++) w.BD[(size_t)e * 18 + 3 * r + q] = Bi[3 * r] * Di[q] + Bi[3 * r + 1] * Di[3 + q] + Bi[3 * r + 2] * Di[6 + q];
    });
    ex.par(w.nPair * 36 + w.P * 6, [&](int idx) {                    // one element per entry of an upper block, one per entry of coefficients
        if (idx < w.nPair * 36) {
            const int pr = idx / 36, r = (idx % 36) / 6, q = idx % 6, s1 = w.pairKey[pr] / LBA_MAX_POSES, s2 = w.pairKey[pr] % LBA_MAX_POSES;
            const int i1 = w.poseIdx[s1], i2 = w.poseIdx[s2];
            if (i1 < 0 || i2 < 0 || (s1 == s2 && r > q)) return;
            double v = 0.0;
            if (s1 == s2) { const int tri = r * 6 - r * (r - 1) / 2 + (q - r); v = w.Hpp[s1 * 27 + tri]; if (r == q) v = v + lambda; }
            for (int a = w.pairStart[pr]; a < w.pairStart[pr + 1]; a++) {
                const int e1 = w.pairE[2 * a], e2 = w.pairE[2 * a + 1];
                if (w.level[e1] || w.level[e2]) continue;
                const double* bd = &w.BD[(size_t)e1 * 18 + 3 * r]; const double* Bj = &w.C[(size_t)e2 * LBA_C + 36 + 3 * q];
                v = v - (bd[0] * Bj[0] + bd[1] * Bj[1] + bd[2] * Bj[2]);
            }
            w.Hs[(size_t)(6 * i1 + r) * n + 6 * i2 + q] = v;
        } else {
            const int s = (idx - w.nPair * 36) / 6, r = (idx - w.nPair * 36) % 6, i = w.poseIdx[s];
            if (i < 0) return;
            double co = 0.0;
            const int pr = w.diagPair[s];
            for (int a = w.pairStart[pr]; a < w.pairStart[pr + 1]; a++) {
                const int e = w.pairE[2 * a]; if (w.level[e]) continue;
                const double* Bi = &w.C[(size_t)e * LBA_C + 36 + 3 * r]; const double* d = &w.db[3 * w.ePt[e]];
                co = co + (Bi[0] * d[0] + Bi[1] * d[1] + Bi[2] * d[2]);
            }
            w.y[6 * i + r] = w.Hpp[s * 27 + 21 + r] - co;           // bschur = b_p - coefficients
        }
    });
    for (int j = 0; j < n; j++) {                                    // LDL^T, column by column; every lane of the column forms D(j) for itself
        ex.par(n - j, [&](int t) {
            const int i = j + t;
            double d = w.Hs[(size_t)j * n + j], v = w.Hs[(size_t)j * n + i];
            for (int k = 0; k < j; k++) { const double ljk = w.Lm[(size_t)k * n + j], dk = w.Dg[k]; d = d - (ljk * dk) * ljk; if (i != j) v = v - (w.Lm[(size_t)k * n + i] * dk) * ljk; }
            if (i == j) w.Dg[j] = d; else w.Lm[(size_t)j * n + i] = v / d;
        });
    }
    ex.par(1, [&](int) { int f = 0; for (int j = 0; j < n; j++) if (w.Dg[j] == 0.0) f = 1; w.isc[LBA_IS_FAIL] = f; });
    if (ex.rdi(&w.isc[LBA_IS_FAIL])) return;
    for (int j = 0; j < n; j++) ex.par(n - j - 1, [&](int t) { const int i = j + 1 + t; w.y[i] = w.y[i] - w.Lm[(size_t)j * n + i] * w.y[j]; });
    ex.par(n, [&](int i) { w.y[i] = w.y[i] / w.Dg[i]; });
    for (int j = n - 1; j > 0; j--) ex.par(j, [&](int i) { w.y[i] = w.y[i] - w.Lm[(size_t)i * n + j] * w.y[j]; });
    ex.par(w.P * 6, [&](int idx) { const int i = w.poseIdx[idx / 6]; if (i >= 0) w.x[idx] = w.y[6 * i + idx % 6]; });
    ex.par(w.nMp, [&](int j) {                                       // cl = bl - sum_i Hpl(i,j)^T xp_i; xl = Dinv * cl
        if (!w.ptAct[j]) return;
        double cl[3] = {w.Hll[j * 9 + 6], w.Hll[j * 9 + 7], w.Hll[j * 9 + 8]};
        for (int a = 0; a < w.ptNF[j]; a++) {
            const int e = w.ptSorted[w.obsStart[j] + a]; if (w.level[e]) continue;
            const double* Bi = &w.C[(size_t)e * LBA_C + 36]; const double* xp = &w.x[6 * w.kfPose[w.eKf[e]]];
            for (int q = 0; q < 3; q++) {
                double t = Bi[q] * -xp[0];
                for (int r = 1; r < 6; r++) t = t + Bi[3 * r + q] * -xp[r];
                cl[q] = cl[q] + t;
            }
        }
        const double* Di = &w.Dinv[j * 9];
        for (int r = 0; r < 3; r++) w.x[6 * w.P + 3 * j + r] = 0.0 + (Di[3 * r] * cl[0] + Di[3 * r + 1] * cl[1] + Di[3 * r + 2] * cl[2]);
    });
}
// SparseOptimizer::update over the index mapping
template <class Ex> SIND_HD inline void lba_update(Ex& ex, const LbaView& w) {
    ex.par(w.P + w.nMp, [&](int idx) {
        if (idx < w.P) { if (w.poseIdx[idx] >= 0) po_oplus(&w.x[6 * idx], w.est[w.poseKf[idx]]); }
        else { const int j = idx - w.P; if (w.ptAct[j]) for (int k = 0; k < 3; k++) w.X[3 * j + k] += w.x[6 * w.P + 3 * j + k]; }
    });
}
// computeScale (optimization_algorithm_levenberg.cpp:182-189) over the whole of x -> sc[LBA_SC_SCALE]
template <class Ex> SIND_HD inline void lba_scale(Ex& ex, const LbaView& w, double lambda) {
    const int nx = 6 * w.P + 3 * w.nMp;
    ex.par(nx, [&](int pos) {                                        // x[j] * (lambda * x[j] + b[j]), poses by rank, then points in ascending mp_id
        double t = 0.0;
        if (pos < 6 * w.P) { const int p = pos / 6, j = pos % 6; if (w.poseIdx[p] >= 0) { const double xj = w.x[pos]; t = xj * (lambda * xj + w.Hpp[p * 27 + 21 + j]); } }
        else { const int q = w.ptOrder[(pos - 6 * w.P) / 3], j = (pos - 6 * w.P) % 3; if (w.ptAct[q]) { const double xj = w.x[6 * w.P + 3 * q + j]; t = xj * (lambda * xj + w.Hll[q * 9 + 6 + j]); } }
        w.term[pos] = t;
    });
    ex.par(1, [&](int) { w.sc[LBA_SC_SCALE] = lba_chain(w.term, nx); });
}
// the classification of :672-702 and :715-743 for every edge: the stored chi2 in double, the depth at the current estimates.  toLevel: setLevel(1); else erase
template <class Ex> SIND_HD inline void lba_classify(Ex& ex, const LbaView& w, bool toLevel) {
    ex.par(w.nObs, [&](int e) {
        const bool stereo = !(w.eObs[4 * e + 2] < 0.0f);
        double Xc[3]; po_map(w.est[w.eKf[e]], &w.X[3 * w.ePt[e]], Xc);
        const bool bad = w.C[(size_t)e * LBA_C + 55] > (stereo ? 7.815 : 5.991) || !(Xc[2] > 0.0);
        if (toLevel) { if (bad) w.level[e] = 1; } else w.erase[e] = bad ? 1 : 0;
    });
    if (toLevel) ex.par(1, [&](int) { int c = 0; for (int e = 0; e < w.nObs; e++) c += w.level[e]; w.isc[LBA_IS_NL1] = c; });
}

// One optimize call as levenberg_optimize's problem (g2o_lm.hpp): each operation is the phases above and then the read of the scalar they left, which on the device is
// a barrier of its own (ex.rd, ex.rdi).  The estimate the stored errors belong to is the workspace's: lba_eval leaves them in C, and nothing rewrites them on a pop.
// computeScale's phases run after the trial's chi2 has been read, as g2o orders the two; they touch neither C nor sc[LBA_SC_CHI]
template <class Ex> struct LbaLm {
    Ex& ex; const LbaView& w; bool robust; int nAct;
    SIND_HD double linearize() { lba_eval(ex, w, robust, true); lba_sums(ex, w, true); return ex.rd(&w.sc[LBA_SC_CHI]); }
    SIND_HD double max_diagonal() { lba_maxdiag(ex, w); return ex.rd(&w.sc[LBA_SC_MAXD]); }
    SIND_HD void push() { lba_push(ex, w); }
    SIND_HD bool solve(double lambda) { lba_solve(ex, w, lambda, nAct); return ex.rdi(&w.isc[LBA_IS_FAIL]) == 0; }
    SIND_HD void update() { lba_update(ex, w); }
    SIND_HD double chi2() { lba_eval(ex, w, robust, false); lba_sums(ex, w, false); return ex.rd(&w.sc[LBA_SC_CHI]); }
    SIND_HD double scale(double lambda) { lba_scale(ex, w, lambda); return ex.rd(&w.sc[LBA_SC_SCALE]); }
    SIND_HD void pop() { lba_pop(ex, w); }
};
// SparseOptimizer::optimize(iterations): x is zeroed here, at buildStructure.  -> iterations run
template <class Ex> SIND_HD inline int lba_optimize(Ex& ex, const LbaView& w, bool robust, int iterations, int nAct, double& chiOut, double& lambdaOut) {
    ex.par(6 * w.P + 3 * w.nMp, [&](int i) { w.x[i] = 0.0; });      // buildStructure
    LbaLm<Ex> lm{ex, w, robust, nAct};
    return levenberg_optimize(lm, iterations, chiOut, lambdaOut);
}

template <class Ex> SIND_HD inline void local_ba(Ex& ex, const LbaView& w) {
    ex.par(w.nKf + w.nMp + w.nObs, [&](int i) {                      // setEstimate(toSE3Quat(GetPose())), toVector3d(GetWorldPos()); every edge at level 0
        if (i < w.nKf) po_from_tcw(&w.Tcw[16 * i], w.est[i]);
        else if (i < w.nKf + w.nMp) { const int j = i - w.nKf; for (int k = 0; k < 3; k++) w.X[3 * j + k] = (double)w.x3Dw[3 * j + k]; }
        else { const int e = i - w.nKf - w.nMp; w.level[e] = 0; w.C[(size_t)e * LBA_C + 55] = 0.0; }
    });
    LbaDiag dg; dg.stages = 0; dg.nLevel1 = 0;
    for (int s = 0; s < 2; s++) { dg.chi2[s] = 0.0; dg.lambda[s] = 0.0; dg.iters[s] = 0; }
    for (int s = 0; s < 2; s++) {
        if (s == 1) {
            if (!w.doMore) break;
            lba_classify(ex, w, true); dg.nLevel1 = ex.rdi(&w.isc[LBA_IS_NL1]);
        }
        lba_activate(ex, w);
        const int nAct = ex.rdi(&w.isc[LBA_IS_NP]), nPts = ex.rdi(&w.isc[LBA_IS_NM]);
        if (nAct + nPts == 0) continue;                              // optimize(): "0 vertices to optimize", -1
        dg.iters[s] = lba_optimize(ex, w, s == 0, s == 0 ? 5 : 10, nAct, dg.chi2[s], dg.lambda[s]);
        dg.stages++;
    }
    lba_classify(ex, w, false);
    ex.par(w.nKf + w.nMp + 1, [&](int i) {
        if (i < w.nKf) { if (w.kfKind[i] == 2) { for (int k = 0; k < 16; k++) w.TcwOut[16 * i + k] = w.Tcw[16 * i + k]; } else po_to_tcw(w.est[i], &w.TcwOut[16 * i]); }
        else if (i < w.nKf + w.nMp) { const int j = i - w.nKf; for (int k = 0; k < 3; k++) w.XOut[3 * j + k] = (float)w.X[3 * j + k]; }
        else *w.diag = dg;
    });
}

// ---------------------------------------------------------------- the host layer both entry points share (local_ba.cpp)
// An item digested: the lists of LbaView and the sizes of its working state.  I: every int array, the inputs first, then the work and output ints (from oLevel on).
struct LbaPlan {
    int nKf = 0, nMp = 0, nObs = 0, P = 0, nPair = 0, nPairE = 0;
    std::vector<int> I;
    size_t oKfKind, oKfPose, oPoseKf, oPtOrder, oObsStart, oEPt, oEKf, oPoseEdgeStart, oPoseEdge, oPtNF, oPtSorted, oPairStart, oPairKey, oPairE, oDiagPair, oLevel, oPoseIdx, oPtAct, oIsc, oErase;
    ItemSizes z;                                                     // the ints that come back: erase; no doubles go in; the head: LbaDiag
};
// -> 0, or what is wrong with the item: 1 a negative count, 2 a NULL array, 3 ids that repeat, 4 an obs_kf out of range, 5 a key frame twice in one point's observations,
// 6 a non-monotone obs_start, 7 an inv_sigma2 that is negative or not finite, 8 a pose or point that is not finite, 9 no key frame of kind 0, 10 a kind outside 0..2
int lba_check(const ::sind_localba_item& q);
extern const char* const lba_check_text[];
// -> SIND_OK or SIND_E_CAPACITY (a limit above); the item has passed lba_check
int lba_plan(const ::sind_localba_item& q, LbaPlan& pl);
// the view of an item over its share of the streams (Fin: Tcw, x3Dw, eObs in this order, filled by lba_fill; Fout: TcwOut, XOut; the head: LbaDiag)
void lba_fill(const ::sind_localba_item& q, const ItemPtrs& p);
void lba_bind(const LbaPlan& pl, int doMore, const PoseOptCam& K, const ItemPtrs& p, LbaView& v);
// an item's outputs from what came back (p: host storage)
void lba_store(const ::sind_localba_item& q, const LbaPlan& pl, const ItemPtrs& p);

}  // namespace sind
