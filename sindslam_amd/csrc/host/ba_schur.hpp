// What Optimizer::LocalBundleAdjustment (local_ba.hpp) and Optimizer::BundleAdjustment (global_ba.hpp) share, written ONCE: the g2o graph of 6-DoF poses and
// marginalised points under binary reprojection edges (mono or stereo), Levenberg-Marquardt over the Schur complement of the points.  ONE source of arithmetic for four
// builds (k_local_ba, the k_gba_phase<> kernels and the two host twins): IEEE FP64 add / mul / div / sqrt everywhere, no contraction (-ffp-contract=off), every sum in
// a stated order, so the four give the same bits.  A correction to one of the literal readings below is made here, once.
// Every phase (evaluate an edge, the ordered sums, Dinv, BDinv, Schur, back-substitution, update, push / pop, computeScale) is a NAMED FUNCTION OF ONE OUTPUT ELEMENT,
// ba_*_elem(const View&, int idx, ...), a template over the view.  Each element writes only its own outputs and reads nothing another element of the same phase writes.
// Who runs the elements is the caller's: local BA's executor (ex.par over one workgroup, or a plain loop) or global BA's runner (one launch per phase, or a plain loop).
// THE THREE REAL DIFFERENCES between the two callers are small inline members of their views, resolved when the template is instantiated (nothing is decided through a
// pointer that may be null at run time):
//   w.level0(e)            is edge e at level 0?  LbaView: level[e] == 0.  GbaView: always, and nothing is read.
//   w.hs_at(i, j, n)       where in Hs entry (row i, column j), i <= j, of Hschur is stored.  LbaView: row-major n x n.  GbaView: the envelope, gba_at(j, i).
//   w.deltas()             the Huber deltas [mono, stereo] handed to ba_edge.  LbaView: NULL = po_delta.  GbaView: delta (sqrt(5.99) for the monocular edge).
// and the loads its chains keep ahead of their additions (View::CHAIN_AHEAD, View::EDGE_AHEAD).
// What exists on one side only stays there: lba_activate, lba_classify and the dense LDL^T (local_ba.hpp); the envelope factor, gba_trisolve and gba_out_elem
// (global_ba.hpp).
//
// RECALLED from pose_opt.hpp (not defined again): PoseQ, po_from_tcw, po_to_tcw, po_quat_to_matrix, po_map, po_exp, po_mul, po_oplus, po_edge_error (the error and chi2
// of both edge types; the stereo cam_project keeps `const float invz`), po_huber, po_delta; from g2o_lm.hpp jtwj_upper, and levenberg_optimize, which both callers drive.
// DEFINED here: ba_inv3, ba_edge (the two binary edges' linearizeOplus and constructQuadraticForm), ba_chain and ba_chain_edges, BaView, the phases ba_*_elem, and the
// part of the host layer both entry points share (ba_plan.cpp).
//
// THE CONTRACT that makes the builds equal, and what it restates of g2o.
// Vertex order (sparse_optimizer.cpp buildIndexMapping :166-190 over the sorted active vertices).  Poses first, then points, each in ascending id, over the vertices
//   active at the level.  Poses are ordered by kf_id.  Points are ordered by mp_id (point ids are all shifted by the same maxKFid+1, so the order is that of mnId).  A
//   vertex without an edge of the requested level is not active (initializeOptimization :206-267: _activeVertices holds a vertex only if it has at least one such
//   edge): it keeps its estimate, and the Hessian indices of the others close up.  A fixed key frame has no index; its edges contribute to the point side only.
// Edge order.  The item's observation order (g2o's internal edge id is the insertion order); mono and stereo edges interleaved as they were inserted.
// buildSystem (block_solver.hpp:502-560; base_binary_edge.hpp:55-115).  Hpp(i,i) and b_i of a pose, Hll(j,j) and b_j of a point are each a sequential FP64 sum from 0
//   over that vertex's active edges in ascending edge order.  Hpl(i,j) has exactly one contributing edge.  activeRobustChi2 is one sequential sum over all active edges
//   in ascending edge order.  The small products take every sum in ascending index order; Omega = invSigma2 * I is applied as one multiplication, as in po_edge_contrib:
//   H(i,j) = sum_d (J[d][i] * W) * J'[d][j] with W = rho1 * invSigma2 (W = invSigma2 without a kernel), for A^T W A, B^T W B and B^T W A alike (A: point, B: pose);
//   b += sum_d J[d][j] * wr[d] with wr = -(invSigma2 * e), times rho1 with a kernel.  Only the upper triangles of Hpp(i,i) and Hll(j,j) are formed and mirrored.
// setLambda (:564-589).  Lambda is added to every diagonal entry of Hpp and Hll.  computeLambdaInit is tau (1e-5) times the largest |diagonal| over all active poses
//   and points, one chain in vertex order with std::max's compare (a NaN diagonal wins).  computeScale runs over the whole of x, poses then points.
// Schur complement, with the loop nest and signs of block_solver.hpp:381-439.  Points are visited in ascending Hessian index.  Dinv = D.inverse() is Eigen's closed-form
//   3 x 3 inverse, DEFINED as ba_inv3: cyclic cofactors over the determinant (det = c00 m00 + c10 m10 + c20 m20).  db = Dinv * b_l.  The point's pose blocks are visited in
//   ascending row i1.  BDinv = Bi * Dinv, formed once per (point, pose).  coefficients_i1 += Bi * db.  For i2 >= i1: Hschur(i1,i2) -= BDinv * Bj^T; only the upper
//   triangle is formed (of a diagonal block too).  Then bschur = b_p - coefficients.  EVERY ENTRY of Hschur and coefficients therefore receives its contributions in
//   ascending point order: one element per entry walks the points both poses see in that order, over the co-observation lists the host layer builds (ba_lists).  Hschur
//   starts as Hpp (with lambda) on the diagonal blocks and 0 elsewhere.
// Reduced system.  The reference uses LinearSolverEigen: Eigen's SimplicialLDLT<Upper> under a scalar AMD ordering, which cannot be reproduced here.  DEFINED instead: an
//   LDL^T in natural order without pivoting; entry (i,j), i >= j, is one function of the finished columns,
//   v = H(j,i); for k < j ascending: v = v - (L(i,k) * D(k)) * L(j,k); D(j) = v at i = j, L(i,j) = v / D(j).  It fails when a pivot equals 0 (SimplicialLDLT's
//   NumericalIssue); x is then untouched.  A NaN pivot does not fail: it poisons tempChi and the step is rejected by g2o_isfinite.  The solves: y(i) -= L(i,j) y(j) in
//   ascending j, y(i) / D(i), y(i) -= L(j,i) y(j) in descending j.  With no active pose the empty factorisation succeeds.  How the matrix is stored and the entries are
//   scheduled is each caller's (dense in local_ba.hpp, a 6 x 6 block envelope in global_ba.hpp).
// Back-substitution (:461-481).  cl = bl - sum_i Hpl(i,j)^T xp_i in ascending pose row, as rightMultiply does it (cl += Hpl^T * (-xp)); xl = 0 + Dinv * cl.
// Update, push and pop.  po_oplus for poses, += for points; push and pop cover all vertices.  Kept literally: after a rejected last trial the edges hold the errors of
//   the REJECTED state.
// x starts as zeros at each buildStructure, that is at iteration 0 of each optimize call (the reference leaves it uninitialised).
//
// UNPINNED PARITY (g2o and Eigen are not available to build or run; restated from the reference's Thirdparty/g2o and Eigen 3.3 as remembered).
//   1. everything pose_opt.hpp lists (Eigen's evaluation order in the small products, -march=native contraction, po_sincos, x * x * x for pow).
//   2. the reduced system: natural-order LDL^T here, SimplicialLDLT under AMD ordering there.
//   3. Eigen's order inside -1./z * tmp * R (here ((-1/z) tmp) R, three terms each, zeros included), inside Dinv * b, Bi * Dinv, Bi * db, BDinv * Bj^T and the 3 x 3 inverse.
//   4. the order of a point's observations: a std::map keyed by pointers there, whatever the caller passes here.
//   5. Hpp(i,i) and Hll(j,j) are accumulated full there (both triangles, which may differ in the last bit); the upper triangle mirrored here.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>
#include "pose_opt.hpp"

namespace sind {

#define LBA_C 56                                                     // doubles per edge: 0..20 pose H (upper, row-major), 21..26 pose b, 27..32 point H (upper), 33..35 point b, 36..53 Hpl [6][3], 54 rho[0], 55 chi2()
enum { BA_SC_CHI = 0, BA_SC_MAXD = 1, BA_SC_SCALE = 2, BA_SC_FAIL = 3, BA_SC_N = 8 };      // the scalars the phases leave in sc; BA_SC_FAIL: global BA's alone (local BA's flag is an int, isc)

// What both views carry of one item: the caller's arrays digested by the plan (read only), the working state up to the reduced system, the outputs.  All pointers are
// host or device alike.  Hs, the storage of Hschur, is here although its shape is each view's (hs_at): with the pointer in GbaView, behind the shared fields, the
// kernels that read it next to Hll .. db or Dg (GbaDinv, the three GbaFactor phases) fetched their arguments with one scalar load more than before.
struct BaView {
    int nKf, nMp, nObs, P, nPair; PoseOptCam K;                      // P: the free poses
    const float* Tcw; const float* x3Dw; const float* eObs;         // [nKf][16], [nMp][3], [nObs][4] = x y uRight invSigma2
    const int* kfPose; const int* poseKf;                            // [nKf] rank of a free key frame by kf_id, else -1; [P] its inverse
    const int* ptOrder; const int* obsStart;                         // [nMp] the points in ascending mp_id; [nMp + 1]
    const int* ePt; const int* eKf;                                  // [nObs]
    const int* poseEdgeStart; const int* poseEdge;                   // [P + 1], [..]: the edges of a free pose in ascending edge order
    const int* ptNF; const int* ptSorted;                            // [nMp], [nObs]: at obsStart[j], ptNF[j] edges of point j into free poses, in ascending pose rank
    const int* pairStart; const int* pairS1; const int* pairS2; const int* pairE;   // [nPair + 1], [nPair] s1 <= s2 (pose ranks), [..][2] = (edge into s1, edge into s2) in ascending point order
    const int* diagPair;                                             // [P] the pair (s, s), -1 without an edge
    int* poseIdx; int* ptAct;                                        // [P] Hessian index or -1; [nMp]
    PoseQ* est; PoseQ* bak; double* X; double* Xbak;                 // [nKf], [nKf], [nMp][3], [nMp][3]
    double* C; double* BD;                                           // [nObs][LBA_C], [nObs][18] BDinv
    double* Hpp; double* Hll; double* Dinv; double* db;              // [P][27] = 21 + 6, [nMp][9] = 6 + 3, [nMp][9], [nMp][3]
    double* Hs; double* Dg; double* y;                               // Hschur as the view stores it (hs_at), [n], [n]; n = 6 * active poses <= 6 P
    double* x; double* sc;                                           // [6 P + 3 nMp] by pose rank and item point, [BA_SC_N]
    double* rho; double* term;                                       // [nObs] rho[0] of an edge, 0 at level 1; [6 P + 3 nMp] the terms of computeScale in vertex order, 0 for an inactive vertex
    float* TcwOut; float* XOut;                                      // [nKf][16], [nMp][3]
};

// Eigen's closed-form inverse of a 3 x 3 (Eigen/src/LU/InverseImpl.h: compute_inverse<.., 3>, cofactor_3x3): inv(i,j) = cofactor(j,i) * (1 / det)
SIND_HD inline double ba_cof(const double m[3][3], int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
}
SIND_HD inline void ba_inv3(const double m[3][3], double inv[3][3]) {
    const double c0 = ba_cof(m, 0, 0), c1 = ba_cof(m, 1, 0), c2 = ba_cof(m, 2, 0);
    const double det = c0 * m[0][0] + c1 * m[1][0] + c2 * m[2][0];
    const double invdet = 1.0 / det;
    inv[0][0] = c0 * invdet; inv[0][1] = c1 * invdet; inv[0][2] = c2 * invdet;
    for (int i = 1; i < 3; i++) for (int j = 0; j < 3; j++) inv[i][j] = ba_cof(m, j, i) * invdet;
}

// One edge: computeError (+ robustify); full: linearizeOplus (types_six_dof_expmap.cpp:103-139, :188-234, as written: divisions by z and z_2) and
// constructQuadraticForm.  poseFree: vertex 1 is not fixed.  c: see LBA_C; not full: c[54] and c[55] alone; !poseFree: the pose entries and Hpl stay unwritten.
// jac (the tests'): _jacobianOplusXi [3][3], _jacobianOplusXj [3][6] and the error [3].  delta: the Huber deltas [mono, stereo] of a caller whose are not po_delta's
// (Optimizer::BundleAdjustment's sqrt(5.99)); NULL: po_delta, local BA's
SIND_HD inline void ba_edge(const PoseQ& P, const PoseOptCam& K, const double X[3], const float* ob, bool robust, bool full, bool poseFree, double* c, double* jac = nullptr, const double* delta = nullptr) {
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

// ---------------------------------------------------------------- the serial chains
// a[0] + a[1] + ... in that order from +0.0, one lane, AHEAD loads in flight before their AHEAD additions so that the chain waits for the adder and not for memory: 8
// are enough while the operands sit in L2 (local BA, the essential graph), over the 10^5 edges of a map it takes 32 (profiles/match_global_ba.txt).  The values lie
// densely; an entry that g2o would not add (an edge at level 1, an inactive vertex) holds +0.0, and s + 0.0 == s for every s such a sum can hold: it starts as +0.0 and
// a sum is -0.0 only if both operands are.  The AHEAD loads and additions are an index sequence and not a loop, so that every build has them as straight-line code
// (the host twins are built at -O2, which leaves such a loop rolled)
template <size_t... K> SIND_HD inline double ba_chain_step(double s, const double* a, std::index_sequence<K...>) {
    const double v[] = {a[K]...};
    ((s = s + v[K]), ...);
    return s;
}
template <int AHEAD> SIND_HD inline double ba_chain(const double* a, int n) {
    double s = 0.0; int i = 0;
    for (; i + AHEAD <= n; i += AHEAD) s = ba_chain_step(s, a + i, std::make_index_sequence<AHEAD>{});
    for (; i < n; i++) s = s + a[i];
    return s;
}
// the same over entry k of the edges of a list (Ck = C + k): AHEAD edges' indices, levels (where the view has levels) and values are fetched before the AHEAD additions
template <class V, size_t... K> SIND_HD inline double ba_chain_edges_step(const V& w, double s, const int* list, const double* Ck, std::index_sequence<K...>) {
    const int e[] = {list[K]...};
    const bool l0[] = {w.level0(e[K])...};
    const double v[] = {Ck[(size_t)e[K] * LBA_C]...};
    ((s = s + (l0[K] ? v[K] : 0.0)), ...);
    return s;
}
template <int AHEAD, class V> SIND_HD inline double ba_chain_edges(const V& w, const int* list, int n, const double* Ck) {
    double s = 0.0; int a = 0;
    for (; a + AHEAD <= n; a += AHEAD) s = ba_chain_edges_step(w, s, list + a, Ck, std::make_index_sequence<AHEAD>{});
    for (; a < n; a++) { const int e = list[a]; s = s + (w.level0(e) ? Ck[(size_t)e * LBA_C] : 0.0); }
    return s;
}

// ---------------------------------------------------------------- the phases, each a function of one output element
// setEstimate(toSE3Quat(GetPose())), toVector3d(GetWorldPos()): i over nKf + nMp
template <class V> SIND_HD inline void ba_init_elem(const V& w, int i) {
    if (i < w.nKf) po_from_tcw(&w.Tcw[16 * i], w.est[i]);
    else { const int j = i - w.nKf; for (int k = 0; k < 3; k++) w.X[3 * j + k] = (double)w.x3Dw[3 * j + k]; }
}
// computeActiveErrors (+ linearizeOplus + constructQuadraticForm if full) of one edge; an edge at level 1 keeps what its last evaluation left in C
template <class V> SIND_HD inline void ba_edge_elem(const V& w, int e, bool robust, bool full) {
    if (!w.level0(e)) { w.rho[e] = 0.0; return; }
    const int kf = w.eKf[e];
    ba_edge(w.est[kf], w.K, &w.X[3 * w.ePt[e]], &w.eObs[4 * e], robust, full, w.kfPose[kf] >= 0, &w.C[(size_t)e * LBA_C], nullptr, w.deltas());
    w.rho[e] = w.C[(size_t)e * LBA_C + 54];
}
// the ordered sums of buildSystem (full: P * 27 + nMp * 9 entries) and, as the last element, activeRobustChi2 -> sc[BA_SC_CHI]
template <class V> SIND_HD inline void ba_sums_elem(const V& w, int idx, bool full) {
    const int nP = full ? w.P * 27 : 0, nM = full ? w.nMp * 9 : 0;
    if (idx < nP) {
        const int p = idx / 27, k = idx % 27;
        w.Hpp[idx] = ba_chain_edges<V::EDGE_AHEAD>(w, w.poseEdge + w.poseEdgeStart[p], w.poseEdgeStart[p + 1] - w.poseEdgeStart[p], w.C + k);
    } else if (idx < nP + nM) {
        const int j = (idx - nP) / 9, k = (idx - nP) % 9;
        double s = 0.0;
        for (int e = w.obsStart[j]; e < w.obsStart[j + 1]; e++) if (w.level0(e)) s = s + w.C[(size_t)e * LBA_C + 27 + k];
        w.Hll[idx - nP] = s;
    } else {
        w.sc[BA_SC_CHI] = ba_chain<V::CHAIN_AHEAD>(w.rho, w.nObs);
    }
}
// the maxDiagonal of computeLambdaInit -> sc[BA_SC_MAXD]: one chain in vertex order (one element)
template <class V> SIND_HD inline void ba_maxdiag_elem(const V& w, int) {
    double maxDiagonal = 0.0;
    const int dp[6] = {0, 6, 11, 15, 18, 20}, dl[3] = {0, 3, 5};
    for (int p = 0; p < w.P; p++) if (w.poseIdx[p] >= 0) for (int j = 0; j < 6; j++) { const double a = fabs(w.Hpp[p * 27 + dp[j]]); maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a; }
    for (int o = 0; o < w.nMp; o++) { const int q = w.ptOrder[o]; if (w.ptAct[q]) for (int j = 0; j < 3; j++) { const double a = fabs(w.Hll[q * 9 + dl[j]]); maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a; } }
    w.sc[BA_SC_MAXD] = maxDiagonal;
}
// push / pop over the vertices: i over nKf + nMp
template <class V> SIND_HD inline void ba_push_elem(const V& w, int i) { if (i < w.nKf) w.bak[i] = w.est[i]; else for (int k = 0; k < 3; k++) w.Xbak[3 * (i - w.nKf) + k] = w.X[3 * (i - w.nKf) + k]; }
template <class V> SIND_HD inline void ba_pop_elem(const V& w, int i) { if (i < w.nKf) w.est[i] = w.bak[i]; else for (int k = 0; k < 3; k++) w.X[3 * (i - w.nKf) + k] = w.Xbak[3 * (i - w.nKf) + k]; }
// Dinv and db of an active point (idx < nMp); one stored entry of Hschur = 0 (the others: as many as the view stores)
template <class V> SIND_HD inline void ba_dinv_elem(const V& w, int idx, double lambda) {
    if (idx >= w.nMp) { w.Hs[idx - w.nMp] = 0.0; return; }
    const int j = idx; if (!w.ptAct[j]) return;
    const double* h = &w.Hll[j * 9];
    const double D[3][3] = {{h[0] + lambda, h[1], h[2]}, {h[1], h[3] + lambda, h[4]}, {h[2], h[4], h[5] + lambda}};
    double inv[3][3]; ba_inv3(D, inv);
    for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) w.Dinv[j * 9 + 3 * r + q] = inv[r][q]; w.db[3 * j + r] = inv[r][0] * h[6] + inv[r][1] * h[7] + inv[r][2] * h[8]; }
}
// BDinv = Bi * Dinv, once per (point, free pose)
template <class V> SIND_HD inline void ba_bdinv_elem(const V& w, int e) {
    if (!w.level0(e) || w.kfPose[w.eKf[e]] < 0) return;
    const double* Bi = &w.C[(size_t)e * LBA_C + 36]; const double* Di = &w.Dinv[w.ePt[e] * 9];
    for (int r = 0; r < 6; r++) for (int q = 0; q < 3; q++) w.BD[(size_t)e * 18 + 3 * r + q] = Bi[3 * r] * Di[q] + Bi[3 * r + 1] * Di[3 + q] + Bi[3 * r + 2] * Di[6 + q];
}
// one entry of an upper block of Hschur (idx < nPair * 36) or of coefficients (the P * 6 after them), each over the points both poses see in ascending point order.
// n = 6 * active poses
template <class V> SIND_HD inline void ba_schur_elem(const V& w, int idx, double lambda, int n) {
    if (idx < w.nPair * 36) {
        const int pr = idx / 36, r = (idx % 36) / 6, q = idx % 6, s1 = w.pairS1[pr], s2 = w.pairS2[pr];
        const int i1 = w.poseIdx[s1], i2 = w.poseIdx[s2];
        if (i1 < 0 || i2 < 0 || (s1 == s2 && r > q)) return;
        double v = 0.0;
        if (s1 == s2) { const int tri = r * 6 - r * (r - 1) / 2 + (q - r); v = w.Hpp[s1 * 27 + tri]; if (r == q) v = v + lambda; }
        for (int a = w.pairStart[pr]; a < w.pairStart[pr + 1]; a++) {
            const int e1 = w.pairE[2 * (size_t)a], e2 = w.pairE[2 * (size_t)a + 1];
            if (!w.level0(e1) || !w.level0(e2)) continue;
            const double* bd = &w.BD[(size_t)e1 * 18 + 3 * r]; const double* Bj = &w.C[(size_t)e2 * LBA_C + 36 + 3 * q];
            v = v - (bd[0] * Bj[0] + bd[1] * Bj[1] + bd[2] * Bj[2]);
        }
        w.Hs[w.hs_at(6 * i1 + r, 6 * i2 + q, n)] = v;
    } else {
        const int s = (idx - w.nPair * 36) / 6, r = (idx - w.nPair * 36) % 6, i = w.poseIdx[s];
        if (i < 0) return;
        double co = 0.0;
        const int pr = w.diagPair[s];
        for (int a = w.pairStart[pr]; a < w.pairStart[pr + 1]; a++) {
            const int e = w.pairE[2 * (size_t)a]; if (!w.level0(e)) continue;
            const double* Bi = &w.C[(size_t)e * LBA_C + 36 + 3 * r]; const double* d = &w.db[3 * w.ePt[e]];
            co = co + (Bi[0] * d[0] + Bi[1] * d[1] + Bi[2] * d[2]);
        }
        w.y[6 * i + r] = w.Hpp[s * 27 + 21 + r] - co;               // bschur = b_p - coefficients
    }
}
// back-substitution of one point: cl = bl - sum_i Hpl(i,j)^T xp_i in ascending pose row; xl = Dinv * cl
template <class V> SIND_HD inline void ba_backsub_elem(const V& w, int j) {
    if (!w.ptAct[j]) return;
    double cl[3] = {w.Hll[j * 9 + 6], w.Hll[j * 9 + 7], w.Hll[j * 9 + 8]};
    for (int a = 0; a < w.ptNF[j]; a++) {
        const int e = w.ptSorted[w.obsStart[j] + a]; if (!w.level0(e)) continue;
        const double* Bi = &w.C[(size_t)e * LBA_C + 36]; const double* xp = &w.x[6 * w.kfPose[w.eKf[e]]];
        for (int q = 0; q < 3; q++) {
            double t = Bi[q] * -xp[0];
            for (int r = 1; r < 6; r++) t = t + Bi[3 * r + q] * -xp[r];
            cl[q] = cl[q] + t;
        }
    }
    const double* Di = &w.Dinv[j * 9];
    for (int r = 0; r < 3; r++) w.x[6 * w.P + 3 * j + r] = 0.0 + (Di[3 * r] * cl[0] + Di[3 * r + 1] * cl[1] + Di[3 * r + 2] * cl[2]);
}
// SparseOptimizer::update of one vertex: idx over P + nMp
template <class V> SIND_HD inline void ba_update_elem(const V& w, int idx) {
    if (idx < w.P) { if (w.poseIdx[idx] >= 0) po_oplus(&w.x[6 * idx], w.est[w.poseKf[idx]]); }
    else { const int j = idx - w.P; if (w.ptAct[j]) for (int k = 0; k < 3; k++) w.X[3 * j + k] += w.x[6 * w.P + 3 * j + k]; }
}
// computeScale (optimization_algorithm_levenberg.cpp:182-189) over the whole of x: one term, x[j] * (lambda * x[j] + b[j]), laid out in vertex order (poses by rank,
// then points in ascending mp_id); then the chain (one element) -> sc[BA_SC_SCALE]
template <class V> SIND_HD inline void ba_scale_term_elem(const V& w, int pos, double lambda) {
    double t = 0.0;
    if (pos < 6 * w.P) { const int p = pos / 6, j = pos % 6; if (w.poseIdx[p] >= 0) { const double xj = w.x[pos]; t = xj * (lambda * xj + w.Hpp[p * 27 + 21 + j]); } }
    else { const int q = w.ptOrder[(pos - 6 * w.P) / 3], j = (pos - 6 * w.P) % 3; if (w.ptAct[q]) { const double xj = w.x[6 * w.P + 3 * q + j]; t = xj * (lambda * xj + w.Hll[q * 9 + 6 + j]); } }
    w.term[pos] = t;
}
template <class V> SIND_HD inline void ba_scale_chain_elem(const V& w, int) { w.sc[BA_SC_SCALE] = ba_chain<V::CHAIN_AHEAD>(w.term, 6 * w.P + 3 * w.nMp); }

// ---------------------------------------------------------------- the host layer both bundle adjustments share (ba_plan.cpp)
// what sind_localba_item and sind_globalba_item have in common
struct BaItem {
    int nKf, nMp, nObs; const int64_t* kfId; const float* Tcw; const int64_t* mpId; const float* x3Dw; const int* obsStart; const int* obsKf;
    const float* obsXy; const float* uRight; const float* invSigma2; float* TcwOut; float* x3DwOut;
};
// nObs is read from obs_start, which ba_check_arrays checks before anyone uses it
template <class Q> inline BaItem ba_item(const Q& q) {
    return {q.n_kf, q.n_mp, (q.n_mp > 0 && q.obs_start) ? q.obs_start[q.n_mp] : 0, q.kf_id, q.Tcw, q.mp_id, q.x3Dw, q.obs_start, q.obs_kf, q.obs_xy, q.u_right, q.inv_sigma2, q.Tcw_out, q.x3Dw_out};
}
// The checks, in the order both callers report: ba_check_arrays -> 0, 1 a negative count, 2 a NULL array (kfNull, mpNull, obsNull: one among the caller's own per key
// frame, per point, per observation), 6 a non-monotone obs_start; then the caller's rules about ids and kinds; then ba_check_obs -> 0, 4 an obs_kf out of range, 5 a key
// frame twice in one point's observations, 7 an inv_sigma2 that is negative or not finite, 8 a pose or point that is not finite
int ba_check_arrays(const BaItem& q, bool kfNull, bool mpNull, bool obsNull);
bool ba_ids_repeat(const int64_t* id, int n);
int ba_check_obs(const BaItem& q);

// An item digested: the lists of BaView and where each lies in I (every int array of the view, the inputs first), the sizes of its share of the streams
struct BaPlan {
    int nKf = 0, nMp = 0, nObs = 0, P = 0, nPair = 0;
    std::vector<int> I;
    size_t oKfPose, oPoseKf, oPtOrder, oObsStart, oEPt, oEKf, oPoseEdgeStart, oPoseEdge, oPtNF, oPtSorted, oPairStart, oPairS1, oPairS2, oPairE, oDiagPair, oPoseIdx, oPtAct;
    ItemSizes z;
    size_t add(const int* p, size_t n) { const size_t o = I.size(); I.insert(I.end(), p, p + n); return o; }
    size_t add(const std::vector<int>& v) { return add(v.data(), v.size()); }
    size_t room(size_t n) { const size_t o = I.size(); I.resize(o + n, 0); return o; }
};
// The counts the limits speak of, before any list is built.  kfPose [nKf]: the rank of a free key frame, else -1 (the caller's rule).  -> ptNF [nMp] the edges of a point
// into free poses, nEdge [P] the edges of a free pose; returns the entries of the co-observation lists, sum over the points of k (k + 1) / 2, k = ptNF
size_t ba_count(const BaItem& q, const std::vector<int>& kfPose, int P, std::vector<int>& ptNF, std::vector<int>& nEdge);
// The lists from kfPose to diagPair into pl (pl.I is started anew; oPoseIdx and oPtAct are the caller's to add).  free_ [P]: kfPose's inverse.  The co-observation lists
// are generated in ascending mp_id and ordered by two stable counting passes over P buckets, by s2 and then by s1: the pairs come out in ascending (s1, s2), the points
// inside a pair in ascending mp_id
void ba_lists(const BaItem& q, const std::vector<int>& kfPose, const std::vector<int>& free_, const std::vector<int>& ptNF, const std::vector<int>& nEdge, size_t total, BaPlan& pl);
// the sizes of the streams both items fill alike; work: the doubles of the working state up to the reduced system and after it (sc .. db; x, term, rho)
void ba_sizes(BaPlan& pl);
// an item's share of Fin: Tcw, x3Dw, eObs in this order
void ba_fill(const BaItem& q, const ItemPtrs& p);
// the view of an item over its share of the streams, up to the reduced system: the counts, K, the inputs, the lists, the outputs and the working state from d on in the
// order sc est bak X Xbak C BD Hpp Hll Dinv db.  -> the cursor: the reduced system (Hs) and Dg y x term rho are the caller's to lay out
double* ba_bind(const BaPlan& pl, const PoseOptCam& K, const ItemPtrs& p, double* d, BaView& v);
// Tcw_out and x3Dw_out from what came back (p: host storage)
void ba_store(const BaItem& q, const BaPlan& pl, const ItemPtrs& p);

}  // namespace sind
