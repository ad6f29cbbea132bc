"""Optimizer::BundleAdjustment (reference src/Optimizer.cc:49-237) restated in Python with NumPy FP64 scalars, in the orders that the head of
sindslam_amd/csrc/host/ba_schur.hpp states.  The graph, the ordered sums, the Schur loop nest, the DENSE LDL^T and the Levenberg-Marquardt loop are localba_ref.Graph's
(the contract is local BA's); what is restated here is what differs: which key frames are free (all but the one with id 0), the Huber deltas (the floats sqrt(5.99) and
sqrt(7.815)), kernels only if robust, one optimize(iterations), no levels.  Because the reduced system is solved by the dense definition here and through the envelope
in the library, bit equality of the two checks the envelope.  Plain sequential loops, for small scenes only."""
from __future__ import annotations

import numpy as np

import localba_ref as R
import poseopt_ref as PR
from poseopt_ref import F, ZERO, f32

DELTA = {False: F(f32(np.sqrt(F(5.99)))), True: F(f32(np.sqrt(F(7.815))))}                        # const float thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815)


def edge(P, K, X, ob, robust, full, pose_free):
    """localba_ref.edge under this function's deltas (the Huber step reads poseopt_ref.DELTA)"""
    keep = PR.DELTA
    PR.DELTA = DELTA
    try:
        return R.edge(P, K, X, ob, robust, full, pose_free)
    finally:
        PR.DELTA = keep


class Graph(R.Graph):
    def __init__(self, it, K):
        super().__init__(dict(it, kf_kind=[1 if int(i) == 0 else 0 for i in it["kf_id"]]), K)
        self.fails = 0

    def evaluate(self, robust, full):
        for e in range(self.n_obs):
            k = self.e_kf[e]
            self.C[e].update(edge(self.est[k], self.K, self.X[self.e_pt[e]], self.ob[e], robust, full, self.kf_pose[k] >= 0))

    def solve(self, lam):
        ok = super().solve(lam)
        self.fails += 0 if ok else 1
        return ok


def global_ba(it, K, iterations=10, robust=False):
    """-> the result dict of ORBmatcher.GlobalBundleAdjustment for one item, without the envelope sizes"""
    with np.errstate(all="ignore"):
        g = Graph(it, K)
        out = dict(n_iters=-1, chi2=ZERO, lambda_=F(-1.0))
        if g.activate() > 0:
            out["n_iters"], out["chi2"], out["lambda_"] = g.optimize(bool(robust), int(iterations))
        out.update(n_active_poses=g.n_act, solver_fail=g.fails, included=np.array(g.pt_act, np.uint8))
        out["Tcw"] = np.array([PR.to_tcw(g.est[k]) for k in range(g.n_kf)], np.float32).reshape(g.n_kf, 4, 4)
        out["x3Dw"] = np.array([[f32(v) for v in g.X[j]] for j in range(g.n_mp)], np.float32).reshape(g.n_mp, 3)
    return out
