// Optimizer::BundleAdjustment (reference src/Optimizer.cc:49-237, what GlobalBundleAdjustemnt forwards to) written out without g2o: one free 6-DoF pose per key frame
// (fixed iff mnId == 0), M marginalised points, one binary reprojection edge (mono or stereo) per observation, Huber kernels only if bRobust, Levenberg-Marquardt over
// the Schur complement of the points, ONE optimize(iterations), no levels and no classification.  ONE source for the host (libsind_host.so: sindh_global_ba,
// global_ba.cpp) and the device (../match_globalba.hip), which give the same bits.  The arithmetic of the graph, the order of every sum and every phase that local BA
// has too are ba_schur.hpp's, whose head states THE CONTRACT in full; this file is what global BA alone has.
//
// A SECOND EXECUTOR SHAPE.  local_ba.hpp runs one item in one workgroup over an executor.  A global BA is one item, an order of magnitude larger, so here every phase
// (ba_schur.hpp's ba_*_elem and this file's gba_*_elem, each A NAMED FUNCTION OF ONE OUTPUT ELEMENT) is wrapped in a small functor (Gba*), and the control flow
// (global_ba<Run>, GbaLm<Run>) runs ON THE HOST for both builds over a runner:
//   run.go(n, phase)   phase(0) ... phase(n - 1), each writing only its own outputs and reading nothing another element of the same phase writes.  Host: a plain loop.
//                      Device: one launch of ceil(n / GBA_THREADS) workgroups, one element per lane; stream order is the only synchronisation between phases.
//   run.tri(w)         the two triangular solves in one workgroup (gba_trisolve<Ex> over SeqExec or WgExec, the pattern of local_ba.hpp).
//   run.fetch(w, sc)   the scalars the phases left in w.sc, for the control flow (device: one copy into page-locked memory and one wait).
// levenberg_optimize (g2o_lm.hpp) is the driver; its problem (GbaLm) enqueues a whole trial (solve, update, chi2, computeScale) behind one fetch and answers the driver's
// four calls from what came back: the values are those of the calls made one by one, because no phase reads a scalar of the control flow but lambda, which the host has.
//
// RECALLED (not defined again): from ba_schur.hpp BaView, ba_edge (its delta argument carries this function's thHuber2D = sqrt(5.99), not local BA's sqrt(5.991)),
// ba_chain and the phases ba_*_elem (edge evaluation, the ordered sums, the max diagonal, push / pop, Dinv, BDinv, Schur, back-substitution, update, computeScale);
// po_to_tcw of pose_opt.hpp; levenberg_optimize of g2o_lm.hpp; SeqExec.
// DEFINED here: GbaView (no levels: every edge is at level 0 and nothing is read to know it; Hschur in the envelope; the deltas of this function; 32 loads ahead in
// the chains), the envelope factor gba_factor_*_elem, gba_trisolve, gba_out_elem, the functors, GbaLm and global_ba.
//
// The call is local BA's stage 1 with another set of free poses, another mono delta, kernels at the caller's choice and the caller's iteration count: on an all-stereo
// item global_ba(iterations = 5, robust) and local_ba(do_more = 0) give the same bits (tests/test_globalba_cpu.py), and the two first linearisations and trials are
// compared there on a mixed window.  A key frame or point without an edge is not active (initializeOptimization) and keeps its estimate; the Hessian indices close up
// (the plan's, once: there are no levels).
//
// THE REDUCED SYSTEM IS AN ENVELOPE (skyline) here, in natural order, in 6 x 6 block rows, as essential_graph.hpp's is in 7 x 7.  Block row I (I = the Hessian index of
// an active pose) is stored from block column first(I) = the smallest Hessian index among the poses that share a point with I, or I itself; every scalar row of it is
// stored from column 6 first(I) to the last column of its diagonal block, H(j,i) and later L(i,j) at (row i, column j), D(j) at (j, j).  Entry (i, j), i >= j:
//   v = H(j,i); for k ascending from max(fcol(i), fcol(j)) to j - 1: v = v - (L(i,k) * D(k)) * L(j,k);  D(j) = v at i = j, L(i,j) = v / D(j)
// For finite values these are the bits of the dense form in local_ba.hpp: a skipped term is a product with an exact zero and v - (+-0) = v for every v a chain can
// hold (essential_graph.hpp gives the induction; the ordered sums never start a chain at -0).  The same failure rule: a zero pivot fails the solve and leaves x
// untouched; a NaN pivot does not fail and poisons the trial.  THE ONE CASE WHERE ENVELOPE AND DENSE DIFFER: a non-finite D(k) (the dense form turns 0 * D(k) into NaN
// where the envelope skips the term); such a trial is rejected either way, but its bits are not claimed.  The per-entry order is the contract, the grouping of the
// entries into launches is not: per block column J, (1) every stored entry of the column takes its terms k < 6 J, (2) the diagonal block is finished, (3) every row below
// takes its at most five terms inside the column and is divided.  The solves: y(i) -= L(i,j) y(j) in ascending j, y(i) / D(i), y(i) -= L(j,i) y(j) in descending j.
//
// NOT OFFERED: a stop flag that flips in the middle of the optimize (iterations = 0 is the flag already set at entry: initializeOptimization, no iteration, the outputs
// are the conversions alone).  UNPINNED PARITY: what ba_schur.hpp lists (g2o / Eigen evaluation orders, SimplicialLDLT under AMD ordering against this envelope, the
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
struct GbaDiag { int iters, nActive, fails; double chi2, lambda; long long env, envDense; };

// The item as both builds see it: BaView and what global BA alone has.  P: key frames with kf_id != 0
struct GbaView : BaView {
    enum { CHAIN_AHEAD = 32, EDGE_AHEAD = 32 };
    int nAct, nActPts, nEnv; double delta[2];                        // nAct: the free key frames with an edge; nEnv: stored entries of the envelope, which is Hs [nEnv]
    const int* first; const int* rowOff;                             // [nAct] first(I); [nAct + 1] where block row I starts in Hs
    const int* colStart; const int* colRow; const int* colLast;      // [nAct + 1], [..]: the block rows I >= J stored in block column J, ascending (J itself first); [nAct] the last of them
    SIND_HD bool level0(int) const { return true; }
    SIND_HD inline size_t hs_at(int i, int j, int) const;           // Hschur(i, j), the upper triangle, lies at (row j, column i)
    SIND_HD const double* deltas() const { return delta; }
};

// where entry (row i, column j) of the envelope lies; fcol(i) <= j <= last column of i's diagonal block
SIND_HD inline int gba_fcol(const GbaView& w, int i) { return 6 * w.first[i / 6]; }
SIND_HD inline size_t gba_at(const GbaView& w, int i, int j) {
    const int I = i / 6, f = w.first[I];
    return (size_t)w.rowOff[I] + (size_t)(i - 6 * I) * (size_t)(6 * (I - f + 1)) + (size_t)(j - 6 * f);
}
SIND_HD inline size_t GbaView::hs_at(int i, int j, int) const { return gba_at(*this, j, i); }

// ---------------------------------------------------------------- the phases of the envelope, each a function of one output element
// The factorisation of block column J in three phases.  (1) idx over 36 * (block rows stored in the column): the entry's terms k < 6 J, ascending
SIND_HD inline void gba_factor_pre_elem(const GbaView& w, int J, int idx) {
    const int I = w.colRow[w.colStart[J] + idx / 36], r = (idx % 36) / 6, c = idx % 6;
    if (I == J && c > r) return;
    const int i = 6 * I + r, j = 6 * J + c, fi = gba_fcol(w, i), fj = gba_fcol(w, j);
    const size_t at = gba_at(w, i, j);
    double v = w.Hs[at];
    const double* Li = &w.Hs[gba_at(w, i, fi)] - fi; const double* Lj = &w.Hs[gba_at(w, j, fj)] - fj;
    for (int k = fi < fj ? fj : fi; k < 6 * J; k++) v = v - (Li[k] * w.Dg[k]) * Lj[k];
    w.Hs[at] = v;
}
// (2) the diagonal block, one element: column by column, the terms inside the block
SIND_HD inline void gba_factor_diag_elem(const GbaView& w, int J, int) {
    for (int c = 0; c < 6; c++) {
        const int j = 6 * J + c;
        for (int r = c; r < 6; r++) {
            const int i = 6 * J + r;
            double v = w.Hs[gba_at(w, i, j)];
            for (int k = 6 * J; k < j; k++) v = v - (w.Hs[gba_at(w, i, k)] * w.Dg[k]) * w.Hs[gba_at(w, j, k)];
            if (i == j) { w.Dg[j] = v; w.Hs[gba_at(w, j, j)] = v; } else w.Hs[gba_at(w, i, j)] = v / w.Dg[j];
        }
    }
}
// (3) idx over 6 * (block rows below the diagonal block): the row's six entries of the column, left to right, each its terms inside the column and the division
SIND_HD inline void gba_factor_post_elem(const GbaView& w, int J, int idx) {
    const int I = w.colRow[w.colStart[J] + 1 + idx / 6], i = 6 * I + idx % 6;
    for (int c = 0; c < 6; c++) {
        const int j = 6 * J + c;
        double v = w.Hs[gba_at(w, i, j)];
        for (int k = 6 * J; k < j; k++) v = v - (w.Hs[gba_at(w, i, k)] * w.Dg[k]) * w.Hs[gba_at(w, j, k)];
        w.Hs[gba_at(w, i, j)] = v / w.Dg[j];
    }
}
// The failure rule and the two solves, in one workgroup (Ex: SeqExec or WgExec): sc[BA_SC_FAIL] = 1 on a zero pivot, x then untouched; else x of the poses
template <class Ex> SIND_HD inline void gba_trisolve(Ex& ex, const GbaView& w) {
    const int n = 6 * w.nAct;
    ex.par(1, [&](int) { double f = 0.0; for (int j = 0; j < n; j++) if (w.Dg[j] == 0.0) f = 1.0; w.sc[BA_SC_FAIL] = f; });
    if (ex.rd(&w.sc[BA_SC_FAIL]) != 0.0) return;
    for (int j = 0; j < n; j++) {
        const int last = 6 * w.colLast[j / 6] + 5;
        ex.par(last - j, [&](int t) { const int i = j + 1 + t; if (gba_fcol(w, i) <= j) w.y[i] = w.y[i] - w.Hs[gba_at(w, i, j)] * w.y[j]; });
    }
    ex.par(n, [&](int i) { w.y[i] = w.y[i] / w.Dg[i]; });
    for (int j = n - 1; j > 0; j--) { const int f = gba_fcol(w, j); ex.par(j - f, [&](int t) { const int i = f + t; w.y[i] = w.y[i] - w.Hs[gba_at(w, j, i)] * w.y[j]; }); }
    ex.par(w.P * 6, [&](int idx) { const int i = w.poseIdx[idx / 6]; if (i >= 0) w.x[idx] = w.y[6 * i + idx % 6]; });
}
// toCvMat(estimate) of every key frame (a round trip through the quaternion, for the fixed one and one without edges too), the float of every point: idx over nKf + nMp
SIND_HD inline void gba_out_elem(const GbaView& w, int i) {
    if (i < w.nKf) po_to_tcw(w.est[i], &w.TcwOut[16 * i]);
    else { const int j = i - w.nKf; for (int k = 0; k < 3; k++) w.XOut[3 * j + k] = (float)w.X[3 * j + k]; }
}

// the phases as what run.go takes: the view by value and the scalars the host chose.  GbaBacksub: after a failed factorisation BlockSolver::solve has returned before
// the back-substitution, so x of the points is untouched too (the flag is the one gba_trisolve left, an earlier phase)
struct GbaInit { GbaView w; SIND_HD void operator()(int i) const { ba_init_elem(w, i); } };
struct GbaZeroX { GbaView w; SIND_HD void operator()(int i) const { w.x[i] = 0.0; } };
struct GbaEdge { GbaView w; bool robust, full; SIND_HD void operator()(int i) const { ba_edge_elem(w, i, robust, full); } };
struct GbaSums { GbaView w; bool full; SIND_HD void operator()(int i) const { ba_sums_elem(w, i, full); } };
struct GbaMaxDiag { GbaView w; SIND_HD void operator()(int i) const { ba_maxdiag_elem(w, i); } };
struct GbaPush { GbaView w; SIND_HD void operator()(int i) const { ba_push_elem(w, i); } };
struct GbaPop { GbaView w; SIND_HD void operator()(int i) const { ba_pop_elem(w, i); } };
struct GbaDinv { GbaView w; double lambda; SIND_HD void operator()(int i) const { ba_dinv_elem(w, i, lambda); } };
struct GbaBDinv { GbaView w; SIND_HD void operator()(int i) const { ba_bdinv_elem(w, i); } };
struct GbaSchur { GbaView w; double lambda; SIND_HD void operator()(int i) const { ba_schur_elem(w, i, lambda, 6 * w.nAct); } };
struct GbaFactorPre { GbaView w; int J; SIND_HD void operator()(int i) const { gba_factor_pre_elem(w, J, i); } };
struct GbaFactorDiag { GbaView w; int J; SIND_HD void operator()(int i) const { gba_factor_diag_elem(w, J, i); } };
struct GbaFactorPost { GbaView w; int J; SIND_HD void operator()(int i) const { gba_factor_post_elem(w, J, i); } };
struct GbaBacksub { GbaView w; SIND_HD void operator()(int i) const { if (w.sc[BA_SC_FAIL] != 0.0) return; ba_backsub_elem(w, i); } };
struct GbaUpdate { GbaView w; SIND_HD void operator()(int i) const { ba_update_elem(w, i); } };
struct GbaScaleTerm { GbaView w; double lambda; SIND_HD void operator()(int i) const { ba_scale_term_elem(w, i, lambda); } };
struct GbaScaleChain { GbaView w; SIND_HD void operator()(int i) const { ba_scale_chain_elem(w, i); } };
struct GbaOut { GbaView w; SIND_HD void operator()(int i) const { gba_out_elem(w, i); } };

// ---------------------------------------------------------------- the control flow, on the host for both builds
// levenberg_optimize's problem.  cs: for each block column, how many block rows it stores (the host's copy of colStart's differences: the launch sizes)
template <class Run> struct GbaLm {
    Run& run; const GbaView& w; const int* cs; bool robust;
    bool first = true; double maxd = 0.0, trialChi = 0.0, trialScale = 0.0; int fails = 0;
    double linearize() {                                             // one wait: chi2 and, before the first iteration, the max diagonal
        run.go(w.nObs, GbaEdge{w, robust, true}); run.go(w.P * 27 + w.nMp * 9 + 1, GbaSums{w, true});
        if (first) run.go(1, GbaMaxDiag{w});
        double sc[BA_SC_N]; run.fetch(w, sc);
        if (first) maxd = sc[BA_SC_MAXD];
        first = false; return sc[BA_SC_CHI];
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
        double sc[BA_SC_N]; run.fetch(w, sc);
        trialChi = sc[BA_SC_CHI]; trialScale = sc[BA_SC_SCALE];
        const bool ok = sc[BA_SC_FAIL] == 0.0;
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
    void fetch(const GbaView& w, double* sc) { for (int k = 0; k < BA_SC_N; k++) sc[k] = w.sc[k]; }
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

// ---------------------------------------------------------------- the host layer both entry points share (global_ba.cpp over ba_plan.cpp)
struct GbaPlan : BaPlan {
    int nAct = 0, nActPts = 0, nEnv = 0; long long envDense = 0;
    std::vector<int> cs;                                             // the block rows per block column
    size_t oFirst, oRowOff, oColStart, oColRow, oColLast;
};
// -> 0, or what is wrong with the item: 1 a negative count, 2 a NULL array, 3 point ids that repeat, 4 an obs_kf out of range, 5 a key frame twice in one point's
// observations, 6 a non-monotone obs_start, 7 an inv_sigma2 that is negative or not finite, 8 a pose or point that is not finite, 9 kf_id not strictly ascending
int gba_check(const ::sind_globalba_item& q);
extern const char* const gba_check_text[];
// -> SIND_OK or SIND_E_CAPACITY (a limit above), decided before any list is built; the item has passed gba_check
int gba_plan(const ::sind_globalba_item& q, GbaPlan& pl);
void gba_bind(const GbaPlan& pl, const PoseOptCam& K, const ItemPtrs& p, GbaView& v);
// an item's outputs from what came back (p: host storage) and the driver's diagnostics
void gba_store(const ::sind_globalba_item& q, const GbaPlan& pl, const ItemPtrs& p, const GbaDiag& dg);

}  // namespace sind
