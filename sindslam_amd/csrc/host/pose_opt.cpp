// Host twin of sind_match_pose_optimize (reference src/Optimizer.cc:239-451): pose_opt.hpp with the plain sequential evaluator, and what the two entry points share:
// the argument check and the copy of one item's results.  Compiled into libsind_hip.so (capi_match_opt.cpp calls the shared part) and into libsind_host.so.
#include <cmath>
#include <cstring>
#include <vector>
#include "pose_opt.hpp"
#include "sind_hip.h"

namespace sind {

void poseopt_store(const ::sind_poseopt_item& q, const PoseOptOut& o, const uint8_t* outlier) {
    *q.n_good = o.nGood; *q.n_rounds = o.nRounds;
    if (q.n < 3) return;
    std::memcpy(q.Tcw_out, o.Tcw, sizeof(o.Tcw)); std::memcpy(q.outlier, outlier, (size_t)q.n);
    if (q.round_iters) std::memcpy(q.round_iters, o.iters, sizeof(o.iters));
    if (q.round_nbad) std::memcpy(q.round_nbad, o.nbad, sizeof(o.nbad));
    if (q.round_pose) std::memcpy(q.round_pose, o.pose, sizeof(o.pose));
    if (q.round_chi2) std::memcpy(q.round_chi2, o.chi2, sizeof(o.chi2));
    if (q.round_lambda) std::memcpy(q.round_lambda, o.lambda, sizeof(o.lambda));
}

// -> 0, or the index (from 1) of the first complaint: 1 negative n, 2 NULL array, 3 inv_sigma2, 4 pose
int poseopt_check(const ::sind_poseopt_item& q) {
    if (q.n < 0) return 1;
    if (!q.Tcw || !q.Tcw_out || !q.n_good || !q.n_rounds || (q.n && (!q.x3Dw || !q.obs_xy || !q.u_right || !q.inv_sigma2 || !q.outlier))) return 2;
    for (int i = 0; i < q.n; i++) if (!(q.inv_sigma2[i] >= 0 && std::isfinite(q.inv_sigma2[i]))) return 3;
    for (int k = 0; k < 16; k++) if (!std::isfinite(q.Tcw[k])) return 4;
    return 0;
}

}  // namespace sind

extern "C" {

// the same items as sind_match_pose_optimize, one after the other on the CPU; fx fy cx cy bf as the handle holds them.  -> 0, or SIND_E_ARG with nothing written
int sindh_pose_optimize(const sind_poseopt_item* items, int B, float fx, float fy, float cx, float cy, float bf) {
    if (B < 0 || (B && !items)) return SIND_E_ARG;
    for (int b = 0; b < B; b++) if (sind::poseopt_check(items[b])) return SIND_E_ARG;
    for (int b = 0; b < B; b++) {
        const sind_poseopt_item& q = items[b];
        std::vector<uint8_t> outlier((size_t)q.n + 1, 0);               // pFrame->mvbOutlier[i] = false (:289, :323)
        sind::PoseOptSeq ev{q.n, q.x3Dw, q.obs_xy, q.u_right, q.inv_sigma2, {(double)fx, (double)fy, (double)cx, (double)cy, (double)bf}, outlier.data()};
        sind::PoseOptOut o;
        sind::pose_optimize(ev, q.n, q.Tcw, o);
        sind::poseopt_store(q, o, outlier.data());
    }
    return SIND_OK;
}

// po_sincos on n arguments (the CPU test compares it with the maths library's)
void sindh_poseopt_sincos(const double* x, int n, double* s, double* c) { for (int i = 0; i < n; i++) sind::po_sincos(x[i], &s[i], &c[i]); }

}  // extern "C"
