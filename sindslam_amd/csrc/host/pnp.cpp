// Host stage of PnPsolver (reference src/PnPsolver.cc): SetRansacParameters (:121-157), the Refine list of a candidate (pnp.hpp), and the host entry points
// over epnp.hpp that the CPU tests and the device-against-host comparison call.  EPnP itself is epnp.hpp, one source for this file and for ../match_pnp.hip.
#include <cmath>
#include <algorithm>
#include <vector>
#include "epnp.hpp"
#include "pnp.hpp"
#include "sind_hip.h"

namespace sind {

int pnp_refine_plan(const int* count, int nIts, int minInliers, int bestCount, bool hasBest, int* refineOfHyp, int* hypOfRefine) {
    int best = bestCount, cur = -1, nRef = 0;
    for (int h = 0; h < nIts; h++) {
        if (count[h] < minInliers) { refineOfHyp[h] = -1; continue; }
        if (count[h] > best) { best = count[h]; cur = nRef; hypOfRefine[nRef++] = h; }
        else if (cur < 0) { if (hasBest) { cur = nRef; hypOfRefine[nRef++] = -1; } else { refineOfHyp[h] = -2; continue; } }
        refineOfHyp[h] = cur;
    }
    return nRef;
}

}  // namespace sind

extern "C" {

// PnPsolver::SetRansacParameters (:121-157): mRansacMinInliers and mRansacMaxIts for n correspondences.  float epsilon, pow, log and ceil as written there.
void sind_pnp_ransac_params(int n, double probability, int min_inliers, int max_its, int min_set, float epsilon, int* min_inliers_out, int* max_its_out) {
    float mRansacEpsilon = epsilon;
    int nMinInliers = (int)(n * mRansacEpsilon);
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    const int mRansacMinInliers = nMinInliers;
    if (n > 0 && mRansacEpsilon < (float)mRansacMinInliers / n) mRansacEpsilon = (float)mRansacMinInliers / n;
    int nIterations;
    if (mRansacMinInliers == n) nIterations = 1;
    else {
        const double it = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(mRansacEpsilon, 3)));
        nIterations = !(it < (double)max_its) ? max_its : it < 1 ? 1 : (int)it;                              // bounded first: the reference converts an unbounded double to int
    }
    if (min_inliers_out) *min_inliers_out = mRansacMinInliers;
    if (max_its_out) *max_its_out = std::max(1, std::min(nIterations, max_its));
}

// compute_pose on n correspondences: x3Dw [n][3], p2d [n][2] FP32 as add_correspondence widens them; R [9], t [3], *rep_error out
void sindh_pnp_pose(int n, const float* x3Dw, const float* p2d, double fu, double fv, double uc, double vc, double* R, double* t, double* rep_error) {
    std::vector<double> buf((size_t)12 * std::max(n, 1));
    double* pws = buf.data(); double* us = pws + 3 * (size_t)n; double* ws = us + 2 * (size_t)n;
    for (int i = 0; i < 3 * n; i++) pws[i] = x3Dw[i];
    for (int i = 0; i < 2 * n; i++) us[i] = p2d[i];
    double mtm[144], Rm[3][3];
    const double e = sind::epnp_compute_pose(n, pws, us, 1, fu, fv, uc, vc, ws, mtm, Rm, t);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = Rm[i][j];
    if (rep_error) *rep_error = e;
}

// CheckInliers (:308-339) of one pose over n correspondences; bits [ceil(n / 64)]; -> mnInliersi
int sindh_pnp_check(int n, const float* x3Dw, const float* p2d, const float* sigma2, float th2, double fu, double fv, double uc, double vc, const double* R, const double* t, uint64_t* bits) {
    int cnt = 0;
    for (int w = 0; w < (n + 63) / 64; w++) bits[w] = 0;
    for (int i = 0; i < n; i++) {
        const float maxError = sigma2[i] * th2;
        if (sind::epnp_is_inlier(R, t, fu, fv, uc, vc, x3Dw[3 * i], x3Dw[3 * i + 1], x3Dw[3 * i + 2], p2d[2 * i], p2d[2 * i + 1], maxError)) { bits[i >> 6] |= 1ull << (i & 63); cnt++; }
    }
    return cnt;
}

int sindh_pnp_refine_plan(const int* count, int n_its, int min_inliers, int best_count, int has_best, int* refine_of_hyp, int* hyp_of_refine) {
    return sind::pnp_refine_plan(count, n_its, min_inliers, best_count, has_best != 0, refine_of_hyp, hyp_of_refine);
}

}  // extern "C"
