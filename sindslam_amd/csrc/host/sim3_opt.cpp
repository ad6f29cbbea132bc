// Host twin of sind_match_sim3_optimize (reference src/Optimizer.cc:1046-1241): sim3_opt.hpp with the plain sequential evaluator, and what the two entry points share:
// the argument check and the copy of one item's results.  Compiled into libsind_hip.so (capi_match_opt.cpp calls the shared part) and into libsind_host.so.
#include <cmath>
#include <cstring>
#include <vector>
#include "sim3_opt.hpp"
#include "sind_hip.h"

namespace sind {

void sim3opt_store(const ::sind_sim3opt_item& q, const Sim3OptOut& o, const uint8_t* removed) {
    std::memcpy(q.q_out, o.q, sizeof(o.q)); std::memcpy(q.t_out, o.t, sizeof(o.t)); *q.s_out = o.s; *q.n_inliers = o.nIn;
    if (q.n) std::memcpy(q.removed, removed, (size_t)q.n);
    if (q.n_bad) *q.n_bad = o.nBad;
    if (q.n_stages) *q.n_stages = o.stages;
    if (q.stage_iters) std::memcpy(q.stage_iters, o.iters, sizeof(o.iters));
    if (q.stage_chi2) std::memcpy(q.stage_chi2, o.chi2, sizeof(o.chi2));
    if (q.stage_lambda) std::memcpy(q.stage_lambda, o.lambda, sizeof(o.lambda));
}

// -> 0, or the index (from 1) of the first complaint: 1 negative n, 2 NULL array, 3 inv_sigma2, 4 the input Sim3 or an intrinsic
int sim3opt_check(const ::sind_sim3opt_item& q) {
    if (q.n < 0) return 1;
    if (!q.K1 || !q.K2 || !q.R12 || !q.t12 || !q.q_out || !q.t_out || !q.s_out || !q.n_inliers) return 2;
    if (q.n && (!q.x3Dc1 || !q.x3Dc2 || !q.obs1_xy || !q.obs2_xy || !q.inv_sigma2_1 || !q.inv_sigma2_2 || !q.removed)) return 2;
    for (int i = 0; i < q.n; i++) if (!(q.inv_sigma2_1[i] >= 0 && std::isfinite(q.inv_sigma2_1[i]) && q.inv_sigma2_2[i] >= 0 && std::isfinite(q.inv_sigma2_2[i]))) return 3;
    if (!std::isfinite(q.s12)) return 4;
    for (int k = 0; k < 9; k++) if (!std::isfinite(q.R12[k])) return 4;
    for (int k = 0; k < 3; k++) if (!std::isfinite(q.t12[k])) return 4;
    for (int k = 0; k < 4; k++) if (!std::isfinite(q.K1[k]) || !std::isfinite(q.K2[k])) return 4;
    return 0;
}

}  // namespace sind

extern "C" {

// the same items as sind_match_sim3_optimize, one after the other on the CPU.  -> 0, or SIND_E_ARG with nothing written
int sindh_sim3_optimize(const sind_sim3opt_item* items, int B, float th2, int fix_scale) {
    if (B < 0 || (B && !items) || !std::isfinite(th2) || th2 < 0) return SIND_E_ARG;
    for (int b = 0; b < B; b++) if (sind::sim3opt_check(items[b])) return SIND_E_ARG;
    for (int b = 0; b < B; b++) {
        const sind_sim3opt_item& q = items[b];
        std::vector<uint8_t> removed((size_t)q.n + 1, 0);
        sind::Sim3OptSeq ev{q.n, q.x3Dc1, q.x3Dc2, q.obs1_xy, q.obs2_xy, q.inv_sigma2_1, q.inv_sigma2_2,
                            {(double)q.K1[0], (double)q.K1[1], (double)q.K1[2], (double)q.K1[3]}, {(double)q.K2[0], (double)q.K2[1], (double)q.K2[2], (double)q.K2[3]},
                            th2, fix_scale != 0, removed.data()};
        sind::Sim3Q S0; sind::s3_from_input(q.s12, q.R12, q.t12, S0);
        sind::Sim3OptOut o;
        sind::sim3_optimize(ev, q.n, S0, fix_scale != 0, o);
        sind::sim3opt_store(q, o, removed.data());
    }
    return SIND_OK;
}

// s3_exp on n arguments (the CPU test compares it with the maths library's)
void sindh_sim3opt_exp(const double* x, int n, double* y) { for (int i = 0; i < n; i++) y[i] = sind::s3_exp(x[i]); }

// both edges' errors and numeric Jacobians [2][7] at one Sim3 (q x y z w, t, s) for one pair (the CPU test compares them with the analytic ones)
void sindh_sim3opt_edges(const double* qts, int fix_scale, const float* K1, const float* K2, const float* X1, const float* X2, const float* o1, const float* o2, double* e12, double* J12, double* e21, double* J21) {
    sind::Sim3Q est; for (int k = 0; k < 4; k++) est.q[k] = qts[k];
    for (int k = 0; k < 3; k++) est.t[k] = qts[4 + k];
    est.s = qts[7];
    sind::Sim3Q T[SIM3OPT_TRANSFORMS], Ti[SIM3OPT_TRANSFORMS];
    for (int k = 0; k < SIM3OPT_TRANSFORMS; k++) sind::s3_perturbed(est, k, fix_scale != 0, T[k], Ti[k]);
    const sind::Sim3Cam c1{(double)K1[0], (double)K1[1], (double)K1[2], (double)K1[3]}, c2{(double)K2[0], (double)K2[1], (double)K2[2], (double)K2[3]};
    const double x1[3] = {(double)X1[0], (double)X1[1], (double)X1[2]}, x2[3] = {(double)X2[0], (double)X2[1], (double)X2[2]};
    const double scalar = 1.0 / (2 * 1e-9);
    sind::s3_edge_error(T[0], c1, x2, (double)o1[0], (double)o1[1], 1.0, e12);
    sind::s3_edge_error(Ti[0], c2, x1, (double)o2[0], (double)o2[1], 1.0, e21);
    for (int d = 0; d < 7; d++) {
        double ep[2], em[2];
        sind::s3_edge_error(T[1 + 2 * d], c1, x2, (double)o1[0], (double)o1[1], 1.0, ep); sind::s3_edge_error(T[2 + 2 * d], c1, x2, (double)o1[0], (double)o1[1], 1.0, em);
        J12[d] = scalar * (ep[0] - em[0]); J12[7 + d] = scalar * (ep[1] - em[1]);
        sind::s3_edge_error(Ti[1 + 2 * d], c2, x1, (double)o2[0], (double)o2[1], 1.0, ep); sind::s3_edge_error(Ti[2 + 2 * d], c2, x1, (double)o2[0], (double)o2[1], 1.0, em);
        J21[d] = scalar * (ep[0] - em[0]); J21[7 + d] = scalar * (ep[1] - em[1]);
    }
}

}  // extern "C"
