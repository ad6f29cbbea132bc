"""Optimizer — Python mirror of the one Optimizer entry point of the reference's tracking thread, Optimizer::PoseOptimization (src/Optimizer.cc:239-451), over
sind_match_pose_optimize, and the chain of Tracking::Relocalization that is built on it (src/Tracking.cc:1460-1524) as the `accept` callback of pnp.relocalization_pnp.

A frame is a dict of per-keypoint arrays: un_xy [N, 2] (mvKeysUn[i].pt), u_right [N] (mvuRight), inv_sigma2 [N] (mvInvLevelSigma2[mvKeysUn[i].octave]), mp i64 [N] (the id of
mvpMapPoints[i], -1 for NULL), x3Dw [N, 3] (GetWorldPos() of that map point; rows without one are not read), Tcw [4, 4] (mTcw), and optionally outlier [N] (mvbOutlier)."""
from __future__ import annotations

import numpy as np


def PoseOptimization(matcher, frame):
    """Optimizer::PoseOptimization(pFrame): flattens the keypoints that hold a map point (ascending i; isBad is not tested, as there), calls
    matcher.PoseOptimization and scatters mvbOutlier back over all keypoints.  `matcher` is an ORBmatcher or anything with its PoseOptimization(items).
    -> (Tcw f32 [4, 4] = what SetPose gets, or mTcw unchanged with fewer than 3 correspondences; mvbOutlier u8 [N]; nGood = nInitialCorrespondences - nBad).
    The frame is not modified."""
    mp = np.asarray(frame["mp"])
    idx = np.nonzero(mp >= 0)[0]
    item = dict(x3Dw=np.asarray(frame["x3Dw"], np.float32)[idx], obs_xy=np.asarray(frame["un_xy"], np.float32)[idx], u_right=np.asarray(frame["u_right"], np.float32)[idx],
                inv_sigma2=np.asarray(frame["inv_sigma2"], np.float32)[idx], Tcw=frame["Tcw"])
    r = matcher.PoseOptimization([item])[0]
    outlier = np.zeros(len(mp), np.uint8) if frame.get("outlier") is None else np.array(frame["outlier"], np.uint8)
    outlier[idx] = r["outlier"] if r["n_rounds"] else 0                 # pFrame->mvbOutlier[i] = false at :289 / :323, before the early return
    return np.array(r["Tcw"], np.float32).reshape(4, 4), outlier, int(r["n_good"])


def search_by_projection_kf(matcher, candidates):
    """The two SearchByProjection(mCurrentFrame, vpCandidateKFs[i], sFound, th, ORBdist) calls of the chain on ORBmatcher.SearchByProjectionKF.  candidates[i]["kf"], per slot of
    the key frame: x3Dw, max_dist, min_dist, valid (pMP && !isBad), angle, desc and mp (the map point's id); the frame carries the searched side's fields (`cur` of
    SearchByProjectionKF: un_xy, octave, angle, desc, grid_start, grid_idx).  -> search(i, frame, sFound, th, ORBdist) -> nadditional, which fills frame["mp"] / ["x3Dw"]"""
    def search(i, frame, sFound, th, ORBdist):
        kf = candidates[i]["kf"]
        ids = np.asarray(kf["mp"])
        k = dict(kf); k["valid"] = (np.asarray(kf["valid"]).astype(bool) & ~np.isin(ids, np.fromiter(sFound, np.int64, len(sFound)))).astype(np.uint8)
        cur = dict(frame); cur["taken"] = (np.asarray(frame["mp"]) >= 0).astype(np.uint8)
        match_of_cur, n = matcher.SearchByProjectionKF([(frame["Tcw"], k, cur)], th, ORBdist)[0]
        j = np.nonzero(match_of_cur >= 0)[0]
        frame["mp"][j] = ids[match_of_cur[j]]; frame["x3Dw"][j] = np.asarray(kf["x3Dw"], np.float32).reshape(-1, 3)[match_of_cur[j]]
        return int(n)
    return search


def relocalization_accept(matcher, frame, candidates, search=None, optimize=None, trace=None):
    """The `accept` callback of pnp.relocalization_pnp: what Tracking::Relocalization does with a pose an iterate returned (src/Tracking.cc:1460-1524).
    frame: as above, plus what `search` reads; it is MODIFIED as mCurrentFrame is (Tcw, mp, x3Dw, outlier).  candidates[i]: match_mp i64 [N] and match_x3Dw [N, 3] =
    vvpMapPointMatches[i] (ids, -1 for NULL, and world positions), and what `search` reads.  search(i, frame, sFound, th, ORBdist) -> nadditional: default
    search_by_projection_kf(matcher, candidates).  optimize(frame) -> (Tcw, mvbOutlier, nGood): default PoseOptimization(matcher, frame).  trace: a list that gets the
    steps taken, in order.  -> accept(i, Tcw, vbInliers, nInliers) -> nGood >= 50"""
    search = search or search_by_projection_kf(matcher, candidates)
    optimize = optimize or (lambda f: PoseOptimization(matcher, f))
    note = (lambda *a: trace.append(a)) if trace is not None else (lambda *a: None)

    def pose_optimization():
        Tcw, outlier, nGood = optimize(frame)
        frame["Tcw"] = Tcw; frame["outlier"] = outlier                   # SetPose, mvbOutlier
        return nGood

    def clear_outliers():
        frame["mp"][frame["outlier"].astype(bool)] = -1                 # :1482-1484, :1510-1512

    def accept(i, Tcw, vbInliers, nInliers):
        c = candidates[i]
        vb = np.asarray(vbInliers, bool)
        frame["Tcw"] = np.array(Tcw, np.float32).reshape(4, 4)          # Tcw.copyTo(mCurrentFrame.mTcw)
        frame["mp"] = np.where(vb, np.asarray(c["match_mp"], np.int64), -1)                                  # :1466-1475
        frame["x3Dw"] = np.array(c["match_x3Dw"], np.float32).reshape(-1, 3)
        if frame.get("outlier") is None:
            frame["outlier"] = np.zeros(len(vb), np.uint8)
        sFound = set(int(v) for v in frame["mp"][vb])
        nGood = pose_optimization(); note("optimize1", nGood)             # :1477
        if nGood < 10:
            note("continue"); return False
        clear_outliers()
        if nGood < 50:
            nadditional = search(i, frame, sFound, 10, 100); note("search1", nadditional)                    # :1489
            if nadditional + nGood >= 50:
                nGood = pose_optimization(); note("optimize2", nGood)     # :1493; the outliers keep their map points here
                if 30 < nGood < 50:
                    sFound = set(int(v) for v in frame["mp"][frame["mp"] >= 0])
                    nadditional = search(i, frame, sFound, 3, 64); note("search2", nadditional)              # :1503
                    if nGood + nadditional >= 50:
                        nGood = pose_optimization(); note("optimize3", nGood)                                 # :1508
                        clear_outliers()
        note("verdict", nGood >= 50)
        return nGood >= 50                                              # :1520
    return accept
