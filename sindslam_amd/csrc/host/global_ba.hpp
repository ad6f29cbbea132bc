// Optimizer::BundleAdjustment (reference src/Optimizer.cc:49-237, what GlobalBundleAdjustemnt forwards to) written out without g2o: one free 6-DoF pose per key frame
// (fixed iff mnId == 0), M marginalised points, one binary reprojection edge (mono or stereo) per observation, Huber kernels only if bRobust, Levenberg-Marquardt over
// the Schur complement of the points, ONE optimize(iterations), no levels and no classification.  ONE source for the host (libsind_host.so: sindh_global_ba,
// global_ba.cpp) and the device (../match_globalba.hip): IEEE FP64 add / mul / div / sqrt on both sides, no contraction (-ffp-contract=off), every sum in a stated order,
// so the two give the same bits.
//
// A SECOND EXECUTOR SHAPE.  local_ba.hpp runs one item in one workgroup; its phases are lambdas over an executor.  A global BA is one item, an order of magnitude larger,
// so here every phase is a NAMED FUNCTION OF ONE OUTPUT ELEMENT, gba_*_elem(const GbaView&, int idx, ...), wrapped in a small functor (Gba*), and the control flow
// (global_ba<Run>, GbaLm<Run>) runs ON THE HOST for both builds over a runner:
//   run.go(n, phase)   phase(0) ... phase(n - 1), each writing only its own outputs and reading nothing another element of the same phase writes.  Host: a plain loop.
//                      Device: one launch of ceil(n / GBA_THREADS) workgroups, one element per lane; stream order is the only synchronisation between phases.
//   run.tri(w)         the two triangular solves in one workgroup (gba_trisolve<Ex> over SeqExec or WgExec, the pattern of local_ba.hpp).
//   run.fetch(w, sc)   the scalars the phases left in w.sc, for the control flow (device: one copy into page-locked memory and one wait).
// levenberg_optimize (g2o_lm.hpp) is the driver; its problem (GbaLm) enqueues a whole trial (solve, update, chi2, computeScale) behind one fetch and answers the driver's
// four calls from what came back: the values are those of the calls made one by one, because no phase reads a scalar of the control flow but lambda, which the host has.
//
// RECALLED (not defined again): lba_edge (the Jacobians as the reference writes them; its delta argument carries this function's thHuber2D = sqrt(5.99), not local BA's
// sqrt(5.991)) and lba_inv3 from local_ba.hpp; the po_* functions of pose_opt.hpp; jtwj_upper and levenberg_optimize of g2o_lm.hpp.  DEFINED here besides the phases:
// gba_chain and gba_chain_edges, lba_chain's sums in lba_chain's order with more loads in flight (below).
//
// THE CONTRACT is local_ba.hpp's (its head states it in full, with what it restates of g2o): vertex order poses by kf_id then points by mp_id; edge order = the item's
// observation order; every block of Hpp, Hll, b, the chi2 and computeScale a sequential FP64 sum from +0.0 in that order; the Schur complement with block_solver.hpp's
// loop nest, so that every entry receives its contributions in ascending point order; back-substitution in ascending pose row; x zeroed at buildStructure; the errors of
// a rejected trial stay in the edges.  A key frame or point without an edge is not active (initializeOptimization) and keeps its estimate; the Hessian indices close up.
// The call is local BA's stage 1 with another set of free poses, another mono delta, kernels at the caller's choice and the caller's iteration count: on an all-stereo
// item global_ba(iterations = 5, robust) and local_ba(do_more = 0) give the same bits (tests/test_globalba_cpu.py).
//
// THE REDUCED SYSTEM IS AN ENVELOPE (skyline) here, in natural order, in 6 x 6 block rows, as essential_graph.hpp's is in 7 x 7.  Block row I (I = the Hessian index of
// an active pose) is stored from block column first(I) = the smallest Hessian index among the poses that share a point with I, or I itself; every scalar row of it is
// stored from column 6 first(I) to the last column of its diagonal block, H(j,i) and later L(i,j) at (row i, column j), D(j) at (j, j).  Entry (i, j), i >= j:
//   v = H(j,i); for k ascending from max(fcol(i), fcol(j)) to j - 1: v = v - (L(i,k) * D(k)) * L(j,k);  D(j) = v at i = j, L(i,j) = v / D(j)
// For finite values these are the bits of the dense definition in local_ba.hpp: a skipped term is a product with an exact zero and v - (+-0) = v for every v a chain can
// hold (essential_graph.hpp gives the induction; the ordered sums never start a chain at -0).  The same failure rule: a zero pivot fails the solve and leaves x
// untouched; a NaN pivot does not fail and poisons the trial.  THE ONE CASE WHERE ENVELOPE AND DENSE DIFFER: a non-finite D(k) (the dense form turns 0 * D(k) into NaN
// where the envelope skips the term); such a trial is rejected either way, but its bits are not claimed.  The per-entry order is the contract, the grouping of the
// entries into launches is not: per block column J, (1) every stored entry of the column takes its terms k < 6 J, (2) the diagonal block is finished, (3) every row below
// takes its at most five terms inside the column and is divided.  The solves: y(i) -= L(i,j) y(j) in ascending j, y(i) / D(i), y(i) -= L(j,i) y(j) in descending j.
//
// NOT OFFERED: a stop flag that flips in the middle of the optimize (iterations = 0 is the flag already set at entry: initializeOptimization, no iteration, the outputs
// are the conversions alone).  UNPINNED PARITY: what local_ba.hpp lists (g2o / Eigen evaluation orders, SimplicialLDLT under AMD ordering against this envelope, the
// order of a point's observations).
// LIMITS (beyond them SIND_E_CAPACITY): GBA_MAX_KF key frames, GBA_MAX_MP points, GBA_MAX_OBS observations, GBA_MAX_PAIRS entries of the co-observation lists (sum over
// the points of k (k + 1) / 2, k = the point's observations in free key frames), GBA_MAX_ENV stored entries of the envelope (36 (I - first(I) + 1) summed over I).
#pragma once
#include <cstdint>
#include "local_ba.hpp"

struct sind_globalba_item;

namespace sind {

#define GBA_MAX_KF 4096
#define GBA_MAX_MP (1 << 20)
#define GBA_MAX_OBS (1 << 22)
#define GBA_MAX_PAIRS (1 << 26)
#define GBA_MAX_ENV (1 << 25)
enum { GBA_SC_CHI = 0, GBA_SC_MAXD = 1, GBA_SC_SCALE = 2, GBA_SC_FAIL = 3, GBA_SC_N = 8 };
struct GbaDiag { int iters, nActive, fails; double chi2, lambda; long long env, envDense; };

// The item as both builds see it: the caller's arrays digested by GbaPlan (read only), the working state, the outputs.  All pointers are host or device alike.
struct GbaView {
    int nKf, nMp, nObs, P, nAct, nActPts, nPair, nEnv; PoseOptCam K; double delta[2];   // P: key frames with kf_id != 0; nAct: those with an edge; nEnv: stored entries
    const float* Tcw; const float* x3Dw; const float* eObs;         // [nKf][16], [nMp][3], [nObs][4] = x y uRight invSigma2
    const int* kfPose; const int* poseKf;                            // [nKf] rank of a free key frame, else -1; [P] its inverse
    const int* ptOrder; const int* obsStart; const int* ePt; const int* eKf;   // [nMp] the points in ascending mp_id; [nMp + 1]; [nObs]; [nObs]
    const int* poseEdgeStart; const int* poseEdge;                   // [P + 1], [..]: the edges of a free pose in ascending edge order
    const int* ptNF; const int* ptSorted;                            // [nMp], [nObs]: at obsStart[j], ptNF[j] edges of point j into free poses, in ascending pose rank
    const int* pairStart; const int* pairS1; const int* pairS2; const int* pairE;   // [nPair + 1], [nPair] s1 <= s2 (pose ranks), [..][2] = (edge into s1, edge into s2) in ascending point order
    const int* diagPair;                                             // [P] the pair (s, s), -1 without an edge
    const int* poseIdx; const int* ptAct;                            // [P] Hessian index or -1; [nMp]
    const int* first; const int* rowOff;                             // [nAct] first(I); [nAct + 1] where block row I starts in E
    const int* colStart; const int* colRow; const int* colLast;      // [nAct + 1], [..]: the block rows I >= J stored in block column J, ascending (J itself first); [nAct] the last of them
    PoseQ* est; PoseQ* bak; double* X; double* Xbak;                 // [nKf], [nKf], [nMp][3], [nMp][3]
    double* C; double* BD;                                           // [nObs][LBA_C], [nObs][18] BDinv
    double* Hpp; double* Hll; double* Dinv; double* db;              // [P][27] = 21 + 6, [nMp][9] = 6 + 3, [nMp][9], [nMp][3]
    double* E; double* Dg; double* y;                                // [nEnv] the envelope, [n], [n]; n = 6 nAct
    double* x; double* sc; double* rho; double* term;                // [6 P + 3 nMp] by pose rank and item point, [GBA_SC_N], [nObs], [6 P + 3 nMp]
    float* TcwOut; float* XOut;                                      // [nKf][16], [nMp][3]
};

// where entry (row i, column j) of the envelope lies; fcol(i) <= j <= last column of i's diagonal block
SIND_HD inline int gba_fcol(const GbaView& w, int i) { return 6 * w.first[i / 6]; }
SIND_HD inline size_t gba_at(const GbaView& w, int i, int j) {
    const int I = i / 6, f = w.first[I];
    return (size_t)w.rowOff[I] + (size_t)(i - 6 * I) * (size_t)(6 * (I - f + 1)) + (size_t)(j - 6 * f);
}

// ---------------------------------------------------------------- the phases, each a function of one output element
// The serial chains.  lba_chain and lba_chain_edges add a[0] + a[1] + ... from +0.0 with eight (four) loads ahead of the additions, which is enough while the operands
// of a local window sit in L2; over the 10^5 edges of a map one lane then waits for memory and not for the adder (profiles/match_global_ba.txt).  The same sums in the
// same order with GBA_AHEAD loads in flight; every edge is at level 0 here, so no level is read
#define GBA_AHEAD 32
SIND_HD inline double gba_chain(const double* a, int n) {
    double s = 0.0; int i = 0;
    for (; i + GBA_AHEAD <= n; i += GBA_AHEAD) {
        double v[GBA_AHEAD];
        for (int k = 0; k < GBA_AHEAD; k++) v[k] = a[i + k];
        for (int k = 0; k < GBA_AHEAD; k++) s = s + v[k];
    }
    for (; i < n; i++) s = s + a[i];
    return s;
}
SIND_HD inline double gba_chain_edges(const int* list, int n, const double* Ck) {
    double s = 0.0; int a = 0;
    for (; a + GBA_AHEAD <= n; a += GBA_AHEAD) {
        double v[GBA_AHEAD];
        for (int k = 0; k < GBA_AHEAD; k++) v[k] = Ck[(size_t)list[a + k] * LBA_C];
        for (int k = 0; k < GBA_AHEAD; k++) s = s + v[k];
    }
    for (; a < n; a++) s = s + Ck[(size_t)list[a] * LBA_C];
    return s;
}
// setEstimate(toSE3Quat(GetPose())), toVector3d(GetWorldPos()): idx over nKf + nMp
SIND_HD inline void gba_init_elem(const GbaView& w, int i) {
    if (i < w.nKf) po_from_tcw(&w.Tcw[16 * i], w.est[i]);
    else { const int j = i - w.nKf; for (int k = 0; k < 3; k++) w.X[3 * j + k] = (double)w.x3Dw[3 * j + k]; }
}
// computeActiveErrors (+ linearizeOplus + constructQuadraticForm if full) of one edge
SIND_HD inline void gba_edge_elem(const GbaView& w, int e, bool robust, bool full) {
    const int kf = w.eKf[e];
    lba_edge(w.est[kf], w.K, &w.X[3 * w.ePt[e]], &w.eObs[4 * e], robust, full, w.kfPose[kf] >= 0, &w.C[(size_t)e * LBA_C], nullptr, w.delta);
    w.rho[e] = w.C[(size_t)e * LBA_C + 54];
}
// the ordered sums of buildSystem (full: P * 27 + nMp * 9 entries) and, as the last element, activeRobustChi2 -> sc[GBA_SC_CHI]
SIND_HD inline void gba_sums_elem(const GbaView& w, int idx, bool full) {
    const int nP = full ? w.P * 27 : 0, nM = full ? w.nMp * 9 : 0;
    if (idx < nP) {
        const int p = idx / 27, k = idx % 27;
        w.Hpp[idx] = gba_chain_edges(w.poseEdge + w.poseEdgeStart[p], w.poseEdgeStart[p + 1] - w.poseEdgeStart[p], w.C + k);
    } else if (idx < nP + nM) {
        const int j = (idx - nP) / 9, k = (idx - nP) % 9;
        double s = 0.0;
        for (int e = w.obsStart[j]; e < w.obsStart[j + 1]; e++) s = s + w.C[(size_t)e * LBA_C + 27 + k];
        w.Hll[idx - nP] = s;
    } else {
        w.sc[GBA_SC_CHI] = gba_chain(w.rho, w.nObs);
    }
}
// the maxDiagonal of computeLambdaInit -> sc[GBA_SC_MAXD]: one chain in vertex order (one element)
SIND_HD inline void gba_maxdiag_elem(const GbaView& w, int) {
    double maxDiagonal = 0.0;
    const int dp[6] = {0, 6, 11, 15, 18, 20}, dl[3] = {0, 3, 5};
    for (int p = 0; p < w.P; p++) if (w.poseIdx[p] >= 0) for (int j = 0; j < 6; j++) { const double a = fabs(w.Hpp[p * 27 + dp[j]]); maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a; }
    for (int o = 0; o < w.nMp; o++) { const int q = w.ptOrder[o]; if (w.ptAct[q]) for (int j = 0; j < 3; j++) { const double a = fabs(w.Hll[q * 9 + dl[j]]); maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a; } }
    w.sc[GBA_SC_MAXD] = maxDiagonal;
}
// push / pop over the vertices: idx over nKf + nMp
SIND_HD inline void gba_push_elem(const GbaView& w, int i) { if (i < w.nKf) w.bak[i] = w.est[i]; else for (int k = 0; k < 3; k++) w.Xbak[3 * (i - w.nKf) + k] = w.X[3 * (i - w.nKf) + k]; }
SIND_HD inline void gba_pop_elem(const GbaView& w, int i) { if (i < w.nKf) w.est[i] = w.bak[i]; else for (int k = 0; k < 3; k++) w.X[3 * (i - w.nKf) + k] = w.Xbak[3 * (i - w.nKf) + k]; }
// Dinv and db of an active point (idx < nMp); one entry of the envelope = 0 (the others)
SIND_HD inline void gba_dinv_elem(const GbaView& w, int idx, double lambda) {
    if (idx >= w.nMp) { w.E[idx - w.nMp] = 0.0; return; }
    const int j = idx; if (!w.ptAct[j]) return;
    const double* h = &w.Hll[j * 9];
    const double D[3][3] = {{h[0] + lambda, h[1], h[2]}, {h[1], h[3] + lambda, h[4]}, {h[2], h[4], h[5] + lambda}};
    double inv[3][3]; lba_inv3(D, inv);
    for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) w.Dinv[j * 9 + 3 * r + q] = inv[r][q]; w.db[3 * j + r] = inv[r][0] * h[6] + inv[r][1] * h[7] + inv[r][2] * h[8]; }
}
// BDinv = Bi * Dinv, once per (point, free pose)
SIND_HD inline void gba_bdinv_elem(const GbaView& w, int e) {
    if (w.kfPose[w.eKf[e]] < 0) return;
    const double* Bi = &w.C[(size_t)e * LBA_C + 36]; const double* Di = &w.Dinv[w.ePt[e] * 9];
    for (int r = 0; r < 6; r++) for (int q = 0; q < 3; q++) w.BD[(size_t)e * 18 + 3 * r + q] = Bi[3 * r] * Di[q] + Bi[3 * r + 1] * Di[3 + q] + Bi[3 * r + 2] * Di[6 + q];
}
// one entry of an upper block of Hschur (idx < nPair * 36) or of coefficients (the P * 6 after them), each over the points both poses see in ascending point order
SIND_HD inline void gba_schur_elem(const GbaView& w, int idx, double lambda) {
    if (idx < w.nPair * 36) {
        const int pr = idx / 36, r = (idx % 36) / 6, q = idx % 6, s1 = w.pairS1[pr], s2 = w.pairS2[pr];
        const int i1 = w.poseIdx[s1], i2 = w.poseIdx[s2];
        if (i1 < 0 || i2 < 0 || (s1 == s2 && r > q)) return;
        double v = 0.0;
        if (s1 == s2) { const int tri = r * 6 - r * (r - 1) / 2 + (q - r); v = w.Hpp[s1 * 27 + tri]; if (r == q) v = v + lambda; }
        for (int a = w.pairStart[pr]; a < w.pairStart[pr + 1]; a++) {
            const int e1 = w.pairE[2 * (size_t)a], e2 = w.pairE[2 * (size_t)a + 1];
            const double* bd = &w.BD[(size_t)e1 * 18 + 3 * r]; const double* Bj = &w.C[(size_t)e2 * LBA_C + 36 + 3 * q];
            v = v - (bd[0] * Bj[0] + bd[1] * Bj[1] + bd[2] * Bj[2]);
        }
        w.E[gba_at(w, 6 * i2 + q, 6 * i1 + r)] = v;                  // Hschur(6 i1 + r, 6 i2 + q), the upper triangle, at (row 6 i2 + q, column 6 i1 + r)
    } else {
        const int s = (idx - w.nPair * 36) / 6, r = (idx - w.nPair * 36) % 6, i = w.poseIdx[s];
        if (i < 0) return;
        double co = 0.0;
        const int pr = w.diagPair[s];
        for (int a = w.pairStart[pr]; a < w.pairStart[pr + 1]; a++) {
            const int e = w.pairE[2 * (size_t)a];
            const double* Bi = &w.C[(size_t)e * LBA_C + 36 + 3 * r]; const double* d = &w.db[3 * w.ePt[e]];
            co = co + (Bi[0] * d[0] + Bi[1] * d[1] + Bi[2] * d[2]);
        }
        w.y[6 * i + r] = w.Hpp[s * 27 + 21 + r] - co;               // bschur = b_p - coefficients
    }
}
// The factorisation of block column J in three phases.  (1) idx over 36 * (block rows stored in the column): the entry's terms k < 6 J, ascending
SIND_HD inline void gba_factor_pre_elem(const GbaView& w, int J, int idx) {
    const int I = w.colRow[w.colStart[J] + idx / 36], r = (idx % 36) / 6, c = idx % 6;
    if (I == J && c > r) return;
    const int i = 6 * I + r, j = 6 * J + c, fi = gba_fcol(w, i), fj = gba_fcol(w, j);
    const size_t at = gba_at(w, i, j);
    double v = w.E[at];
    const double* Li = &w.E[gba_at(w, i, fi)] - fi; const double* Lj = &w.E[gba_at(w, j, fj)] - fj;
    for (int k = fi < fj ? fj : fi; k < 6 * J; k++) v = v - (Li[k] * w.Dg[k]) * Lj[k];
    w.E[at] = v;
}
// (2) the diagonal block, one element: column by column, the terms inside the block
SIND_HD inline void gba_factor_diag_elem(const GbaView& w, int J, int) {
    for (int c = 0; c < 6; c++) {
        const int j = 6 * J + c;
        for (int r = c; r < 6; r++) {
            const int i = 6 * J + r;
            double v = w.E[gba_at(w, i, j)];
            for (int k = 6 * J; k < j; k++) v = v - (w.E[gba_at(w, i, k)] * w.Dg[k]) * w.E[gba_at(w, j, k)];
            if (i == j) { w.Dg[j] = v; w.E[gba_at(w, j, j)] = v; } else w.E[gba_at(w, i, j)] = v / w.Dg[j];
        }
    }
}
// (3) idx over 6 * (block rows below the diagonal block): the row's six entries of the column, left to right, each its terms inside the column and the division
SIND_HD inline void gba_factor_post_elem(const GbaView& w, int J, int idx) {
    const int I = w.colRow[w.colStart[J] + 1 + idx / 6], i = 6 * I + idx % 6;
    for (int c = 0; c < 6; c++) {
        const int j = 6 * J + c;
        double v = w.E[gba_at(w, i, j)];
        for (int k = 6 * J; k < j; k++) v = v - (w.E[gba_at(w, i, k)] * w.Dg[k]) * w.E[gba_at(w, j, k)];
        w.E[gba_at(w, i, j)] = v / w.Dg[j];
    }
}
// The failure rule and the two solves, in one workgroup (Ex: SeqExec or WgExec): sc[GBA_SC_FAIL] = 1 on a zero pivot, x then untouched; else x of the poses
template <class Ex> SIND_HD inline void gba_trisolve(Ex& ex, const GbaView& w) {
    const int n = 6 * w.nAct;
    ex.par(1, [&](int) { double f = 0.0; for (int j = 0; j < n; j++) if (w.Dg[j] == 0.0) f = 1.0; w.sc[GBA_SC_FAIL] = f; });
    if (ex.rd(&w.sc[GBA_SC_FAIL]) != 0.0) return;
    for (int j = 0; j < n; j++) {
        const int last = 6 * w.colLast[j / 6] + 5;
        ex.par(last - j, [&](int t) { const int i = j + 1 + t; if (gba_fcol(w, i) <= j) w.y[i] = w.y[i] - w.E[gba_at(w, i, j)] * w.y[j]; });
    }
    ex.par(n, [&](int i) { w.y[i] = w.y[i] / w.Dg[i]; });
    for (int j = n - 1; j > 0; j--) { const int f = gba_fcol(w, j); ex.par(j - f, [&](int t) { const int i = f + t; w.y[i] = w.y[i] - w.E[gba_at(w, j, i)] * w.y[j]; }); }
    ex.par(w.P * 6, [&](int idx) { const int i = w.poseIdx[idx / 6]; if (i >= 0) w.x[idx] = w.y[6 * i + idx % 6]; });
}
// back-substitution of one point: cl = bl - sum_i Hpl(i,j)^T xp_i in ascending pose row; xl = Dinv * cl.  After a failed factorisation BlockSolver::solve has returned
// before this part: x of the points is untouched too (the flag is the one gba_trisolve left, an earlier phase)
SIND_HD inline void gba_backsub_elem(const GbaView& w, int j) {
    if (w.sc[GBA_SC_FAIL] != 0.0 || !w.ptAct[j]) return;
    double cl[3] = {w.Hll[j * 9 + 6], w.Hll[j * 9 + 7], w.Hll[j * 9 + 8]};
    for (int a = 0; a < w.ptNF[j]; a++) {
        const int e = w.ptSorted[w.obsStart[j] + a];
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
SIND_HD inline void gba_update_elem(const GbaView& w, int idx) {
    if (idx < w.P) { if (w.poseIdx[idx] >= 0) po_oplus(&w.x[6 * idx], w.est[w.poseKf[idx]]); }
    else { const int j = idx - w.P; if (w.ptAct[j]) for (int k = 0; k < 3; k++) w.X[3 * j + k] += w.x[6 * w.P + 3 * j + k]; }
}
// one term of computeScale, x[j] * (lambda * x[j] + b[j]), laid out in vertex order (poses by rank, then points in ascending mp_id); then the chain (one element)
SIND_HD inline void gba_scale_term_elem(const GbaView& w, int pos, double lambda) {
    double t = 0.0;
    if (pos < 6 * w.P) { const int p = pos / 6, j = pos % 6; if (w.poseIdx[p] >= 0) { const double xj = w.x[pos]; t = xj * (lambda * xj + w.Hpp[p * 27 + 21 + j]); } }
    else { const int q = w.ptOrder[(pos - 6 * w.P) / 3], j = (pos - 6 * w.P) % 3; if (w.ptAct[q]) { const double xj = w.x[6 * w.P + 3 * q + j]; t = xj * (lambda * xj + w.Hll[q * 9 + 6 + j]); } }
    w.term[pos] = t;
}
SIND_HD inline void gba_scale_chain_elem(const GbaView& w, int) { w.sc[GBA_SC_SCALE] = gba_chain(w.term, 6 * w.P + 3 * w.nMp); }
// toCvMat(estimate) of every key frame (a round trip through the quaternion, for the fixed one and one without edges too), the float of every point: idx over nKf + nMp
SIND_HD inline void gba_out_elem(const GbaView& w, int i) {
    if (i < w.nKf) po_to_tcw(w.est[i], &w.TcwOut[16 * i]);
    else { const int j = i - w.nKf; for (int k = 0; k < 3; k++) w.XOut[3 * j + k] = (float)w.X[3 * j + k]; }
}

// the phases as what run.go takes: the view by value and the scalars the host chose
struct GbaInit { GbaView w; SIND_HD void operator()(int i) const { gba_init_elem(w, i); } };
struct GbaZeroX { GbaView w; SIND_HD void operator()(int i) const { w.x[i] = 0.0; } };
struct GbaEdge { GbaView w; bool robust, full; SIND_HD void operator()(int i) const { gba_edge_elem(w, i, robust, full); } };
struct GbaSums { GbaView w; bool full; SIND_HD void operator()(int i) const { gba_sums_elem(w, i, full); } };
struct GbaMaxDiag { GbaView w; SIND_HD void operator()(int i) const { gba_maxdiag_elem(w, i); } };
struct GbaPush { GbaView w; SIND_HD void operator()(int i) const { gba_push_elem(w, i); } };
struct GbaPop { GbaView w; SIND_HD void operator()(int i) const { gba_pop_elem(w, i); } };
struct GbaDinv { GbaView w; double lambda; SIND_HD void operator()(int i) const { gba_dinv_elem(w, i, lambda); } };
struct GbaBDinv { GbaView w; SIND_HD void operator()(int i) const { gba_bdinv_elem(w, i); } };
struct GbaSchur { GbaView w; double lambda; SIND_HD void operator()(int i) const { gba_schur_elem(w, i, lambda); } };
struct GbaFactorPre { GbaView w; int J; SIND_HD void operator()(int i) const { gba_factor_pre_elem(w, J, i); } };
struct GbaFactorDiag { GbaView w; int J; SIND_HD void operator()(int i) const { gba_factor_diag_elem(w, J, i); } };
struct GbaFactorPost { GbaView w; int J; SIND_HD void operator()(int i) const { gba_factor_post_elem(w, J, i); } };
struct GbaBacksub { GbaView w; SIND_HD void operator()(int i) const { gba_backsub_elem(w, i); } };
struct GbaUpdate { GbaView w; SIND_HD void operator()(int i) const { gba_update_elem(w, i); } };
struct GbaScaleTerm { GbaView w; double lambda; SIND_HD void operator()(int i) const { gba_scale_term_elem(w, i, lambda); } };
struct GbaScaleChain { GbaView w; SIND_HD void operator()(int i) const { gba_scale_chain_elem(w, i); } };
struct GbaOut { GbaView w; SIND_HD void operator()(int i) const { gba_out_elem(w, i); } };

// ---------------------------------------------------------------- the control flow, on the host for both builds
// levenberg_optimize's problem.  cs: for each block column, how many block rows it stores (the host's copy of colStart's differences: the launch sizes)
template <class Run> struct GbaLm {
    Run& run; const GbaView& w; const int* cs; bool robust;
    bool first = true; double maxd = 0.0, trialChi = 0.0, trialScale = 0.0; int fails = 0;
    double linearize() {                                             // one wait: chi2 and, before the first iteration, the max diagonal
        run.go(w.nObs, GbaEdge{w, robust, true}); run.go(w.P * 27 + w.nMp * 9 + 1, GbaSums{w, true});
        if (first) run.go(1, GbaMaxDiag{w});
        double sc[GBA_SC_N]; run.fetch(w, sc);
        if (first) maxd = sc[GBA_SC_MAXD];
        first = false; return sc[GBA_SC_CHI];
    }
    double max_diagonal() const { return maxd; }
    void push() { run.go(w.nKf + w.nMp, GbaPush{w}); }
    bool solve(double lambda) {                                      // one wait: the whole trial.  A failed solve leaves x as it was, and update still applies it, as in g2o
        run.go(w.nMp + w.nEnv, GbaDinv{w, lambda}); run.go(w.nObs, GbaBDinv{w}); run.go(w.nPair * 36 + w.P * 6, GbaSchur{w, lambda});
        for (int J = 0; J < w.nAct; J++) { run.go(36 * cs[J], GbaFactorPre{w, J}); run.go(1, GbaFactorDiag{w, J}); run.go(6 * (cs[J] - 1), GbaFactorPost{w, J}); }
        run.tri(w);
        run.go(w.nMp, GbaBacksub{w});
        run.go(w.P + w.nMp, GbaUpdate{w});
        run.go(w.nObs, GbaEdge{w, robust, false}); run.go(1, GbaSums{w, false});
        run.go(6 * w.P + 3 * w.nMp, GbaScaleTerm{w, lambda}); run.go(1, GbaScaleChain{w});
        double sc[GBA_SC_N]; run.fetch(w, sc);
        trialChi = sc[GBA_SC_CHI]; trialScale = sc[GBA_SC_SCALE];
        const bool ok = sc[GBA_SC_FAIL] == 0.0;
        if (!ok) fails++;
        return ok;
    }
    void update() {}
    double chi2() const { return trialChi; }
    double scale(double) const { return trialScale; }
    void pop() { run.go(w.nKf + w.nMp, GbaPop{w}); }
};

// the plain runner of the host twin
struct GbaSeqRun {
    template <class Ph> void go(int n, const Ph& ph) { for (int i = 0; i < n; i++) ph(i); }
    void tri(const GbaView& w) { SeqExec ex; gba_trisolve(ex, w); }
    void fetch(const GbaView& w, double* sc) { for (int k = 0; k < GBA_SC_N; k++) sc[k] = w.sc[k]; }
};

// the call: the conversions, initializeOptimization (the plan's active sets), one optimize(iterations), the conversions back
template <class Run> inline void global_ba(Run& run, const GbaView& w, const int* cs, int iterations, bool robust, GbaDiag& dg) {
    run.go(w.nKf + w.nMp, GbaInit{w});
    dg.iters = -1; dg.chi2 = 0.0; dg.lambda = -1.0; dg.nActive = w.nAct; dg.fails = 0;
    if (w.nAct + w.nActPts > 0) {                                    // else optimize(): "0 vertices to optimize", -1
        run.go(6 * w.P + 3 * w.nMp, GbaZeroX{w});                    // buildStructure
        GbaLm<Run> lm{run, w, cs, robust};
        dg.iters = levenberg_optimize(lm, iterations, dg.chi2, dg.lambda);
        dg.fails = lm.fails;
    }
    run.go(w.nKf + w.nMp, GbaOut{w});
}

// ---------------------------------------------------------------- the host layer both entry points share (global_ba.cpp)
struct GbaPlan {
    int nKf = 0, nMp = 0, nObs = 0, P = 0, nAct = 0, nActPts = 0, nPair = 0, nEnv = 0; long long envDense = 0;
    std::vector<int> I, cs;                                          // every int array of the view; the block rows per block column
    size_t oKfPose, oPoseKf, oPtOrder, oObsStart, oEPt, oEKf, oPoseEdgeStart, oPoseEdge, oPtNF, oPtSorted, oPairStart, oPairS1, oPairS2, oPairE, oDiagPair, oPoseIdx, oPtAct, oFirst, oRowOff, oColStart, oColRow, oColLast;
    ItemSizes z;
};
// -> 0, or what is wrong with the item: 1 a negative count, 2 a NULL array, 3 point ids that repeat, 4 an obs_kf out of range, 5 a key frame twice in one point's
// observations, 6 a non-monotone obs_start, 7 an inv_sigma2 that is negative or not finite, 8 a pose or point that is not finite, 9 kf_id not strictly ascending
int gba_check(const ::sind_globalba_item& q);
extern const char* const gba_check_text[];
// -> SIND_OK or SIND_E_CAPACITY (a limit above), decided before any list is built; the item has passed gba_check
int gba_plan(const ::sind_globalba_item& q, GbaPlan& pl);
void gba_fill(const ::sind_globalba_item& q, const ItemPtrs& p);
void gba_bind(const GbaPlan& pl, const PoseOptCam& K, const ItemPtrs& p, GbaView& v);
// an item's outputs from what came back (p: host storage) and the driver's diagnostics
void gba_store(const ::sind_globalba_item& q, const GbaPlan& pl, const ItemPtrs& p, const GbaDiag& dg);

}  // namespace sind
