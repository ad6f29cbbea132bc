// Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:506-778) written out without g2o: P free 6-DoF poses, fixed poses, M marginalised points, binary
// reprojection edges (mono or stereo), Levenberg-Marquardt over the Schur complement of the points, optimize(5) with Huber kernels, the outliers moved to level 1,
// optimize(10) without kernels, the final classification.  ONE source for the host (libsind_host.so: sindh_local_ba, local_ba.cpp) and the device
// (../match_localba.hip: k_local_ba), which give the same bits.  The arithmetic of the graph, the order of every sum and every phase that global BA has too are
// ba_schur.hpp's, whose head states THE CONTRACT in full; this file is what local BA alone has.  The control flow (local_ba<Ex>) is a template over an executor, which
// only says who runs the elements of a phase:
//   ex.par(n, f)   f(0) ... f(n - 1), each writing only its own outputs and reading nothing another element of the same phase writes.  Host: a plain loop.  Device:
//                  the lanes of one workgroup stride over the elements, then one barrier.
//   ex.rd(p)       a scalar that a phase left in the workspace, read for the control flow (device: every lane reads it, then a barrier, so the next phase may rewrite it).
// The Levenberg-Marquardt scalars are computed by every lane from the same workspace values, so the control flow is uniform over the workgroup.
//
// RECALLED (not defined again): from ba_schur.hpp BaView, ba_edge, ba_chain and the phases ba_*_elem (edge evaluation, the ordered sums, the max diagonal, push / pop,
// Dinv, BDinv, Schur, back-substitution, update, computeScale); from pose_opt.hpp po_map, po_to_tcw; from g2o_lm.hpp levenberg_optimize.
// DEFINED here: LbaView (the levels: an edge at level 1 is skipped by every phase; Hschur dense; po_delta's Huber deltas), lba_activate, lba_classify, the dense LDL^T
// and its solves in lba_solve, the grouping of the phases into the driver's operations (LbaLm), local_ba and the output rule for kind 2.
//
// WHAT IS LOCAL BA'S OWN in the contract.
// Levels.  A vertex with no level-0 edge left in stage 2 is not active: it keeps its estimate, and the Hessian indices of the others close up (lba_activate).  An edge
//   at level 1 keeps the error of its last evaluation in stage 1, and the final classification reads that.
// Reduced system.  The dense 6P x 6P matrix, Hs row-major (upper), L(i,k) at Lm[k * n + i]: column by column, every lane of the column forms D(j) for itself.  With
//   P = 0 (every pose fixed) the empty factorisation succeeds.  A NaN pivot: 0 * D(k) is NaN here where global BA's envelope skips the term (global_ba.hpp).
// Kept literally: after a rejected last trial the edges hold the errors of the REJECTED state; the classification reads those, while isDepthPositive reads the
//   restored estimates.
// The function.  Stage 1: optimize(5), Huber on every edge, deltas the floats sqrt(5.991) and sqrt(7.815).  Classification: chi2() > 5.991 (mono) or > 7.815 (stereo) or
//   !isDepthPositive() -> level 1; the compares are in double (not in float as in PoseOptimization); a NaN chi2 compares false, a NaN depth is not positive.  Kernels
//   removed from all edges.  Stage 2: initializeOptimization(0), optimize(10); an optimize with no active vertex does nothing (g2o returns -1) and is not counted in
//   n_stages.  The final classification gives vToErase.  Local key frames (kind 0 and 1) get toCvMat(estimate), a round trip through the quaternion; fixed cameras
//   (kind 2) are not written (their output rows are the input); points get the float of the estimate.  do_more = 0 is bDoMore = false: the stop flag seen after stage 1;
//   the level changes and stage 2 are then skipped.
// NOT OFFERED: a stop flag that flips in the middle of an optimize (terminate() is always false here).  pMP->isBad() during the call cannot happen: the item is a copy.
// UNPINNED PARITY: what ba_schur.hpp lists.
// LIMITS (beyond them SIND_E_CAPACITY): LBA_MAX_POSES free poses, LBA_MAX_KF key frames, LBA_MAX_MP points, LBA_MAX_OBS observations, LBA_MAX_PAIRS entries of the
// co-observation lists (sum over the points of k (k + 1) / 2, k = the point's observations in free poses).
#pragma once
#include "ba_schur.hpp"

struct sind_localba_item;

namespace sind {

#define LBA_MAX_POSES 256
#define LBA_MAX_KF 4096
#define LBA_MAX_MP 65536
#define LBA_MAX_OBS (1 << 20)
#define LBA_MAX_PAIRS (1 << 24)
enum { LBA_IS_NP = 0, LBA_IS_NM = 1, LBA_IS_FAIL = 2, LBA_IS_NL1 = 3, LBA_IS_N = 8 };
struct LbaDiag { double chi2[2], lambda[2]; int stages, iters[2], nLevel1; };

// One item as both executors see it: BaView and what local BA alone has
struct LbaView : BaView {
    enum { CHAIN_AHEAD = 8, EDGE_AHEAD = 4 };
    int doMore; const int* kfKind;                                   // [nKf] the item's kind
    double* Lm;                                                      // [n][n] L(i,k) at k * n + i; Hs: [n][n] row-major (upper); n = 6 * active poses <= 6 P
    int* level; int* isc;                                            // [nObs], [LBA_IS_N]
    int* erase; LbaDiag* diag;                                       // [nObs], [1]
    SIND_HD bool level0(int e) const { return level[e] == 0; }
    SIND_HD size_t hs_at(int i, int j, int n) const { return (size_t)i * n + j; }
    SIND_HD const double* deltas() const { return nullptr; }
};

// ---------------------------------------------------------------- the phases as the executor runs them
// computeActiveErrors (+ linearizeOplus + constructQuadraticForm if full) over the level-0 edges
template <class Ex> SIND_HD inline void lba_eval(Ex& ex, const LbaView& w, bool robust, bool full) { ex.par(w.nObs, [&](int e) { ba_edge_elem(w, e, robust, full); }); }
// the ordered sums of buildSystem (full) and activeRobustChi2 -> sc[BA_SC_CHI]
template <class Ex> SIND_HD inline void lba_sums(Ex& ex, const LbaView& w, bool full) { ex.par((full ? w.P * 27 + w.nMp * 9 : 0) + 1, [&](int idx) { ba_sums_elem(w, idx, full); }); }
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
// the maxDiagonal of computeLambdaInit -> sc[BA_SC_MAXD]
template <class Ex> SIND_HD inline void lba_maxdiag(Ex& ex, const LbaView& w) { ex.par(1, [&](int i) { ba_maxdiag_elem(w, i); }); }
// push / pop over the vertices
template <class Ex> SIND_HD inline void lba_push(Ex& ex, const LbaView& w) { ex.par(w.nKf + w.nMp, [&](int i) { ba_push_elem(w, i); }); }
template <class Ex> SIND_HD inline void lba_pop(Ex& ex, const LbaView& w) { ex.par(w.nKf + w.nMp, [&](int i) { ba_pop_elem(w, i); }); }
// BlockSolver::solve with setLambda(lambda): Schur complement, LDL^T, the two solves, back-substitution -> x; isc[LBA_IS_FAIL] != 0: a zero pivot, x untouched
template <class Ex> SIND_HD inline void lba_solve(Ex& ex, const LbaView& w, double lambda, int nAct) {
    const int n = 6 * nAct;
    ex.par(w.nMp + n * n, [&](int idx) { ba_dinv_elem(w, idx, lambda); });
    ex.par(w.nObs, [&](int e) { ba_bdinv_elem(w, e); });
    ex.par(w.nPair * 36 + w.P * 6, [&](int idx) { ba_schur_elem(w, idx, lambda, n); });
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
    ex.par(w.nMp, [&](int j) { ba_backsub_elem(w, j); });
}
// SparseOptimizer::update over the index mapping
template <class Ex> SIND_HD inline void lba_update(Ex& ex, const LbaView& w) { ex.par(w.P + w.nMp, [&](int idx) { ba_update_elem(w, idx); }); }
// computeScale over the whole of x -> sc[BA_SC_SCALE]
template <class Ex> SIND_HD inline void lba_scale(Ex& ex, const LbaView& w, double lambda) {
    ex.par(6 * w.P + 3 * w.nMp, [&](int pos) { ba_scale_term_elem(w, pos, lambda); });
    ex.par(1, [&](int i) { ba_scale_chain_elem(w, i); });
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
// computeScale's phases run after the trial's chi2 has been read, as g2o orders the two; they touch neither C nor sc[BA_SC_CHI]
template <class Ex> struct LbaLm {
    Ex& ex; const LbaView& w; bool robust; int nAct;
    SIND_HD double linearize() { lba_eval(ex, w, robust, true); lba_sums(ex, w, true); return ex.rd(&w.sc[BA_SC_CHI]); }
    SIND_HD double max_diagonal() { lba_maxdiag(ex, w); return ex.rd(&w.sc[BA_SC_MAXD]); }
    SIND_HD void push() { lba_push(ex, w); }
    SIND_HD bool solve(double lambda) { lba_solve(ex, w, lambda, nAct); return ex.rdi(&w.isc[LBA_IS_FAIL]) == 0; }
    SIND_HD void update() { lba_update(ex, w); }
    SIND_HD double chi2() { lba_eval(ex, w, robust, false); lba_sums(ex, w, false); return ex.rd(&w.sc[BA_SC_CHI]); }
    SIND_HD double scale(double lambda) { lba_scale(ex, w, lambda); return ex.rd(&w.sc[BA_SC_SCALE]); }
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
        if (i < w.nKf + w.nMp) ba_init_elem(w, i);
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

// ---------------------------------------------------------------- the host layer both entry points share (local_ba.cpp over ba_plan.cpp)
// An item digested: BaPlan, and where local BA's own int arrays lie in I (the work and output ints from oLevel on)
struct LbaPlan : BaPlan {
    size_t oKfKind, oLevel, oIsc, oErase;                            // z: the ints that come back: erase; no doubles go in; the head: LbaDiag
};
// -> 0, or what is wrong with the item: 1 a negative count, 2 a NULL array, 3 ids that repeat, 4 an obs_kf out of range, 5 a key frame twice in one point's observations,
// 6 a non-monotone obs_start, 7 an inv_sigma2 that is negative or not finite, 8 a pose or point that is not finite, 9 no key frame of kind 0, 10 a kind outside 0..2
int lba_check(const ::sind_localba_item& q);
extern const char* const lba_check_text[];
// -> SIND_OK or SIND_E_CAPACITY (a limit above), decided before any list is built; the item has passed lba_check
int lba_plan(const ::sind_localba_item& q, LbaPlan& pl);
// the view of an item over its share of the streams (Fin: filled by ba_fill; Fout: TcwOut, XOut; the head: LbaDiag)
void lba_bind(const LbaPlan& pl, int doMore, const PoseOptCam& K, const ItemPtrs& p, LbaView& v);
// an item's outputs from what came back (p: host storage)
void lba_store(const ::sind_localba_item& q, const LbaPlan& pl, const ItemPtrs& p);

}  // namespace sind
