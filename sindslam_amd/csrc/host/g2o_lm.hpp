// What PoseOptimization (pose_opt.hpp), OptimizeSim3 (sim3_opt.hpp) and the bundle adjustments (ba_schur.hpp) share of g2o and Eigen, restated ONCE: Eigen's quaternion
// product, the upper triangle of J^T W J, Eigen's pivoted LDLT behind LinearSolverDense, the dense N x N system of a single free vertex, and the control flow of
// SparseOptimizer::optimize over OptimizationAlgorithmLevenberg::solve.  Everything is SIND_HD inline: the host twins and the device kernels compile the same text,
// IEEE FP64 on both sides and no contraction (-ffp-contract=off), so they give the same bits.  A correction to one of the literal readings below is made here, once.
//
// UNPINNED PARITY.  g2o and Eigen are not available to build or run; what follows is restated from the reference's Thirdparty/g2o and from Eigen 3.3 as remembered.
//   1. Eigen's LDLT (ldlt_inplace<Lower>::unblocked with its pivoting and sign tracking, isPositive(), solve with the pseudo-inverse of D at tolerance 1 / highest).
//   2. pow(2 rho - 1, 3) of the lambda update as x * x * x.
// Kept literally, for all three optimizers (levenberg_optimize):
//   - the solver's x is DEFINED to start as zeros (Solver::resizeVector leaves it uninitialised in a release build; update() reads it after a failed first solve) and
//     is never cleared by the driver: when it is zeroed is the caller's (pose: never, across iterations and rounds; Sim3: never, across both stages; local BA: at each
//     optimize, where buildStructure reallocates it);
//   - after a rejected trial the edges still hold the errors of the REJECTED estimate: pop() restores the vertices, nobody recomputes the errors, and the callers'
//     classifications read those.  The problem notes the estimate its stored errors belong to whenever it evaluates;
//   - _currentLambda is -1 until computeLambdaInit has run, which is what a call with no iteration reports.
// At the end, host only: what the host layers of local BA and the essential graph share (SeqExec, ItemSizes, ItemPtrs, HostItem).
#pragma once
#include <cmath>
#include <cfloat>
#include <cstddef>
#include <vector>
#include "peac_fit.hpp"                                              // SIND_HD

namespace sind {

// Eigen's quaternion product a * b (Eigen/src/Geometry/Quaternion.h, quat_product), coefficients x y z w; neither is normalised here: SE3Quat::operator* does that
// afterwards, Sim3::operator* never.  r must not alias a or b
SIND_HD inline void po_quat_mul(const double a[4], const double b[4], double r[4]) {
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// The upper triangle (row-major) of J^T (W I) J, J of two rows or, if `third`, of three: Omega = invSigma2 * I (times rho[1]) applied as one multiplication per row, every
// sum in ascending row order.  NOT SHARED, because the arithmetic differs between the callers: the Jacobians themselves (po_edge_contrib multiplies by invz and invz_2,
// ba_edge divides by z and z_2, as the reference's two source files do), the right-hand sides (rho1 * (A^T (s e)) there, A^T (-(s e) rho1) in ba_edge and
// s3_edge_contrib) and local BA's B^T W A, which is not a triangle
template <int R, int N> SIND_HD inline void jtwj_upper(const double (&J)[R][N], double W, bool third, double* c) {
    static_assert(R == 2 || R == 3, "two rows, or three of which the last may be unused");
    int k = 0;
    for (int i = 0; i < N; i++) for (int j = i; j < N; j++) {
        double h = (J[0][i] * W) * J[0][j] + (J[1][i] * W) * J[1][j];
        if (R == 3 && third) h = h + (J[R - 1][i] * W) * J[R - 1][j];
        c[k++] = h;
    }
}

// ---------------------------------------------------------------- LinearSolverDense::solve (linear_solver_dense.h:104-112): Eigen::LDLT, isPositive(), solve
// H: the full symmetric N x N (only its lower triangle is read).  -> false if !isPositive(); x is then untouched
template <int N> SIND_HD inline bool ldlt_solve(const double (&Hin)[N][N], const double (&b)[N], double (&x)[N]) {
    double m[N][N]; int tr[N]; double temp[N];
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) m[i][j] = Hin[i][j];
    int sign = 0;                                                    // ZeroSign 0, PositiveSemiDef 1, NegativeSemiDef -1, Indefinite 2
    for (int k = 0; k < N; k++) {
        int big = k; double best = fabs(m[k][k]);                    // mat.diagonal().tail(size-k).cwiseAbs().maxCoeff(&index): the first maximum
        for (int i = k + 1; i < N; i++) if (fabs(m[i][i]) > best) { best = fabs(m[i][i]); big = i; }
        tr[k] = big;
        if (k != big) {
            for (int j = 0; j < k; j++) { const double t = m[k][j]; m[k][j] = m[big][j]; m[big][j] = t; }
            for (int i = big + 1; i < N; i++) { const double t = m[i][k]; m[i][k] = m[i][big]; m[i][big] = t; }
            { const double t = m[k][k]; m[k][k] = m[big][big]; m[big][big] = t; }
            for (int i = k + 1; i < big; i++) { const double t = m[i][k]; m[i][k] = m[big][i]; m[big][i] = t; }
        }
        const int rs = N - k - 1;
        if (k > 0) {
            for (int j = 0; j < k; j++) temp[j] = m[j][j] * m[k][j];
            double a = 0.0;
            for (int j = 0; j < k; j++) a = a + m[k][j] * temp[j];
            m[k][k] -= a;
            for (int i = k + 1; i < N; i++) { double v = 0.0; for (int j = 0; j < k; j++) v = v + m[i][j] * temp[j]; m[i][k] -= v; }
        }
        const double realAkk = m[k][k];
        const bool valid = fabs(realAkk) > 0.0;
        if (k == 0 && !valid) { sign = 0; for (int j = 0; j < N; j++) tr[j] = j; break; }       // the entire matrix is zero
        if (rs > 0 && valid) for (int i = k + 1; i < N; i++) m[i][k] /= realAkk;
        if (sign == 1) { if (realAkk < 0.0) sign = 2; }
        else if (sign == -1) { if (realAkk > 0.0) sign = 2; }
        else if (sign == 0) { if (realAkk > 0.0) sign = 1; else if (realAkk < 0.0) sign = -1; }
    }
    if (!(sign == 1 || sign == 0)) return false;                     // isPositive()
    double d[N];
    for (int i = 0; i < N; i++) d[i] = b[i];
    for (int k = 0; k < N; k++) { const double t = d[k]; d[k] = d[tr[k]]; d[tr[k]] = t; }     // dst = P b
    for (int j = 0; j < N; j++) for (int i = j + 1; i < N; i++) d[i] -= d[j] * m[i][j];        // L^-1
    const double tol = 1.0 / DBL_MAX;                                // D^+ : RealScalar(1) / NumTraits<RealScalar>::highest()
    for (int i = 0; i < N; i++) { if (fabs(m[i][i]) > tol) d[i] /= m[i][i]; else d[i] = 0.0; }
    for (int j = N - 1; j >= 0; j--) for (int i = j - 1; i >= 0; i--) d[i] -= d[j] * m[j][i];  // L^-T
    for (int k = N - 1; k >= 0; k--) { const double t = d[k]; d[k] = d[tr[k]]; d[tr[k]] = t; } // P^T
    for (int i = 0; i < N; i++) x[i] = d[i];
    return true;
}

// The system of a graph whose one free vertex has N dimensions (pose: 6, Sim3: 7), as the BlockSolver holds it: H, b and the solver's x, which is the caller's
template <int N> struct DenseSystem {
    double H[N][N], b[N]; double (&x)[N];
    SIND_HD explicit DenseSystem(double (&x_)[N]) : x(x_) {}
    // from the ordered sums over the edges: the N (N + 1) / 2 entries of the upper triangle of H (row-major), then the N of b
    SIND_HD void load(const double* S) {
        int k = 0;
        for (int a = 0; a < N; a++) for (int c = a; c < N; c++) { H[a][c] = S[k]; H[c][a] = S[k]; k++; }
        for (int j = 0; j < N; j++) b[j] = S[k + j];
    }
    SIND_HD double max_diagonal() const {                            // computeLambdaInit's loop (:166-180), std::max's compare: a NaN diagonal wins
        double maxDiagonal = 0.0;
        for (int j = 0; j < N; j++) { const double a = fabs(H[j][j]); maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a; }
        return maxDiagonal;
    }
    SIND_HD bool solve(double lambda) {                              // setLambda(_currentLambda, true), solve, restoreDiagonal: H itself is never changed
        double Hl[N][N];
        for (int a = 0; a < N; a++) for (int c = 0; c < N; c++) Hl[a][c] = (a == c) ? H[a][c] + lambda : H[a][c];
        return ldlt_solve<N>(Hl, b, x);
    }
    SIND_HD double scale(double lambda) const {                      // computeScale's sum (:182-189)
        double scale = 0.0;
        for (int j = 0; j < N; j++) scale += x[j] * (lambda * x[j] + b[j]);
        return scale;
    }
};

// ---------------------------------------------------------------- SparseOptimizer::optimize(iterations) (sparse_optimizer.cpp:357-414) over
// OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-164).  -> the iterations run; chi2: the last accepted activeRobustChi2; lambda: see above
// Pr, the problem: what a step means for one optimizer.  Its operations, in the order g2o calls them:
//   double linearize()          computeActiveErrors, activeRobustChi2 (returned), linearizeOplus and buildSystem at the current estimate
//   double max_diagonal()       the largest |diagonal entry| of the Hessian over the active vertices, in vertex order
//   void   push()               the estimates of the active vertices onto their stacks
//   bool   solve(lambda)        setLambda, _solver->solve() into x, restoreDiagonal; false: the factorisation failed and x is what it was
//   void   update()             oplus of x on every active vertex
//   double chi2()               computeActiveErrors and activeRobustChi2 at the trial estimate
//   double scale(lambda)        sum over x of x[j] * (lambda * x[j] + b[j])
//   void   pop()                the estimates back from the stacks (the errors in the edges stay those of the trial)
// On the device every lane runs this with the same values, so the flow is uniform over the workgroup and every barrier inside an operation is reached by all lanes.
// Always inlined: each optimizer calls it from one place, and its phases stay in the caller's one function as they were when each optimizer had the loop written out.
// userLambdaInit: setUserLambdaInit; computeLambdaInit (:166-180) returns it when it is > 0 and never looks at the diagonal then.  The three optimizers above leave it 0
template <class Pr> SIND_HD inline __attribute__((always_inline)) int levenberg_optimize(Pr& pr, int iterations, double& chi2, double& lambdaOut, double userLambdaInit = 0.0) {
    double lambda = -1.0, ni = 2.0, currentChi = 0.0;                // _currentLambda, _ni
    int cj = 0, nBadLM = 0; bool ok = true;
    for (int i = 0; i < iterations && ok; i++) {                     // sparse_optimizer.cpp:376-414
        currentChi = pr.linearize();
        double tempChi = currentChi; const double iniChi = currentChi;
        if (i == 0) { lambda = (userLambdaInit > 0) ? userLambdaInit : 1e-5 * pr.max_diagonal(); ni = 2.0; nBadLM = 0; }      // computeLambdaInit (:166-180), _tau = 1e-5
        double rho = 0.0; int qmax = 0;
        do {
            pr.push();
            const bool ok2 = pr.solve(lambda);
            pr.update();                                             // update(_solver->x())
            tempChi = pr.chi2();
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = pr.scale(lambda);                         // computeScale (:182-189)
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && fabs(tempChi) <= DBL_MAX) {               // g2o_isfinite
                const double w = 2 * rho - 1;
                double alpha = 1. - w * w * w;
                alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;         // (std::min)(alpha, _goodStepUpperScale)
                const double scaleFactor = (1. / 3. < alpha) ? alpha : 1. / 3.;   // (std::max)(_goodStepLowerScale, alpha)
                lambda *= scaleFactor; ni = 2; currentChi = tempChi; // discardTop
            } else {
                lambda *= ni; ni *= 2; pr.pop();
            }
            qmax++;
        } while (rho < 0 && qmax < 10);                              // _maxTrialsAfterFailure
        bool terminate = false;
        if (qmax == 10 || rho == 0) terminate = true;
        else {
            if ((iniChi - currentChi) * 1e3 < iniChi) nBadLM++; else nBadLM = 0;       // Stop criterium (Raul)
            if (nBadLM >= 3) terminate = true;
        }
        ok = !terminate; cj++;
    }
    chi2 = currentChi; lambdaOut = lambda;
    return cj;
}

// ---------------------------------------------------------------- what LocalBundleAdjustment and OptimizeEssentialGraph share of their host layer: a call's items lie
// one after the other in a few streams (the device call, ../match_handle.hpp: PackedItems) or each in vectors of its own (the host twins: HostItem)
// The plain sequential executor of the host twins (the device's is WgExec, ../match_device.hpp)
struct SeqExec {
    template <class F> void par(int n, F f) { for (int i = 0; i < n; i++) f(i); }
    double rd(const double* p) { return *p; }
    int rdi(const int* p) { return *p; }
};

// What one item takes of each stream, in elements: LbaPlan and EssPlan report it in this shape
struct ItemSizes {
    size_t ints = 0, intsOutAt = 0, intsOut = 0;                     // every int array; [intsOutAt, intsOutAt + intsOut) of them comes back (local BA's erase flags)
    size_t floatsIn = 0, floatsOut = 0, doublesIn = 0;               // doublesIn: the Sim3 maps of the essential graph
    size_t head = 0, work = 0;                                       // doubles that come back (the diagnostics first); doubles of the working state, room for the head included
};
// where an item's share of each stream starts, host or device alike.  The host twins keep the head where the working state has room for it: head == D
struct ItemPtrs { int* I; float* Fin; float* Fout; double* Din; double* head; double* D; };

// an item bound to host storage: the caller digests it into pl (no workspace yet), store() allocates the workspace
template <class Plan, class View> struct HostItem {
    Plan pl; std::vector<float> Fin, Fout; std::vector<double> Din, D; ItemPtrs p{}; View v;
    void store() {
        const ItemSizes& z = pl.z;
        Fin.assign(z.floatsIn + 1, 0.f); Fout.assign(z.floatsOut + 1, 0.f); Din.assign(z.doublesIn + 1, 0.0); D.assign(z.work + 1, 0.0);
        p = ItemPtrs{pl.I.data(), Fin.data(), Fout.data(), Din.data(), D.data(), D.data()};
    }
};

}  // namespace sind
