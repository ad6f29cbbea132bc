"""Mapping — Python mirror of the arithmetic the local mapper and the loop closer do on the map points themselves, over sind_match_triangulate and
sind_match_update_points: LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452), the point updates of ProcessNewKeyFrame (:139-161) and SearchInNeighbors
(:517-530), and MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (src/MapPoint.cc:242-307, :330-371) wherever the reference calls the pair.

The map is the plain dicts of optimizer.py (local_ba_graph), with optional keys more.  A key frame: Tcw [4, 4], Twc [4, 4] (GetPoseInverse(); formed from Tcw in float as
SetPose does where absent), un_xy [N, 2] (mvKeysUn), xy [N, 2] (mvKeys, the distorted keys UnprojectStereo reads; un_xy where absent), octave i32 [N], u_right [N], depth
[N] (mvDepth), desc u8 [N, 32] (mDescriptors), node i32 [N] and angle [N] (for SearchForTriangulation), mp i64 [N], bad, covisible.  A map point: x3Dw [3], obs {kf id:
slot}, bad, ref_kf (mpRefKF), and what the updates write: desc u8 [32] (mDescriptor), normal [3] (mNormalVector), max_dist, min_dist (mfMaxDistance, mfMinDistance: the
members, before the 1.2f / 0.8f factors, as the searches take them).  A point's observations are walked in ascending key-frame id (the reference: a std::map keyed by
pointers).  `matcher` is an ORBmatcher or anything with its SearchForTriangulation, Triangulate and UpdateMapPoints and its K5 = (fx, fy, cx, cy, bf)."""
from __future__ import annotations

import numpy as np

MAX_POINTS_PER_ITEM = 65536                                            # the limit of one sind_mappoints_item


def pose_inverse(kf):
    """GetPoseInverse() of a key-frame dict: its Twc, or Twc formed from Tcw in float as SetPose forms it"""
    if kf.get("Twc") is not None:
        return np.asarray(kf["Twc"], np.float32).reshape(4, 4)
    Tcw = np.asarray(kf["Tcw"], np.float32).reshape(4, 4)
    Twc = np.eye(4, dtype=np.float32); Twc[:3, :3] = Tcw[:3, :3].T; Twc[:3, 3] = -(Tcw[:3, :3].T @ Tcw[:3, 3])
    return Twc


def camera_centre(kf):
    """GetCameraCenter(): column 3 of Twc"""
    return pose_inverse(kf)[:3, 3].copy()


def compute_f12(kf1, kf2, K5):
    """LocalMapping::ComputeF12(pKF1, pKF2) (src/LocalMapping.cc:536-556): K^-T [t12]x R12 K^-1 with R12 = R1w R2w^T, t12 = -R12 t2w + t1w.  Formed in FP64 and rounded to
    FP32: F12 is an input of the search, which both the library and its references read as given; this is not a bit-level restatement of cv::Mat::inv."""
    T1 = np.asarray(kf1["Tcw"], np.float64).reshape(4, 4); T2 = np.asarray(kf2["Tcw"], np.float64).reshape(4, 4)
    R12 = T1[:3, :3] @ T2[:3, :3].T; t12 = -R12 @ T2[:3, 3] + T1[:3, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K = np.array([[K5[0], 0, K5[2]], [0, K5[1], K5[3]], [0, 0, 1]], np.float64); Ki = np.linalg.inv(K)
    return (Ki.T @ tx @ R12 @ Ki).astype(np.float32)


def _norm3(v):
    """cv::norm of three floats assigned to a float: squares summed in FP64 in order, (float)sqrt"""
    s = np.float64(0)
    for x in np.asarray(v, np.float32):
        s = s + np.float64(x) * np.float64(x)
    return np.float32(np.sqrt(s))


def _tri_side(kf):
    n = len(kf["octave"])
    return dict(xy=np.asarray(kf.get("xy", kf["un_xy"]), np.float32), un_xy=np.asarray(kf["un_xy"], np.float32), octave=np.asarray(kf["octave"], np.int32),
                u_right=np.asarray(kf["u_right"], np.float32), depth=np.asarray(kf["depth"], np.float32) if kf.get("depth") is not None else np.full(n, -1, np.float32))


def _search_side(kf):
    return dict(node=kf["node"], has_mp=(np.asarray(kf["mp"]) >= 0).astype(np.uint8), un_xy=kf["un_xy"], octave=kf["octave"], angle=kf["angle"], u_right=kf["u_right"], desc=kf["desc"])


def neighbours_for_triangulation(matcher, kf_id, keyframes, nn=10):
    """:213-253 for the RGB-D tracker: GetBestCovisibilityKeyFrames(nn) and the baseline test `baseline < pKF2->mb` -> the neighbours that are kept, in order"""
    cur = keyframes[kf_id]
    mb = np.float32(matcher.K5[4]) / np.float32(matcher.K5[0])
    Ow1 = camera_centre(cur)
    return [k for k in list(cur["covisible"])[:nn] if not _norm3(camera_centre(keyframes[k]) - Ow1) < mb]


def _add_new_point(kf_id, k, idx1, idx2, X, keyframes, mappoints):
    """:434-440: new MapPoint(x3D, mpCurrentKeyFrame, mpMap), both AddObservation, both AddMapPoint -> the new id"""
    m = max(mappoints) + 1 if mappoints else 0
    mappoints[m] = dict(x3Dw=np.array(X, np.float32), obs={kf_id: int(idx1), k: int(idx2)}, bad=False, ref_kf=kf_id, first_kf=kf_id)
    keyframes[kf_id]["mp"][idx1] = m; keyframes[k]["mp"][idx2] = m
    return m


def create_new_map_points(matcher, kf_id, keyframes, mappoints, nn=10):
    """LocalMapping::CreateNewMapPoints whole (src/LocalMapping.cc:207-452), for the RGB-D tracker (nn = 10, the stereo baseline test): the neighbours and the baseline test,
    SearchForTriangulation for all kept neighbours in ONE call, Triangulate in ONE call, then the tail in (neighbour, idx1) order: new point, both AddObservation, both
    AddMapPoint, and one update_map_points over the new points.  The map IS modified.  -> the ids of the new points, in the order they were created.

    Why the batch is exact.  The reference searches neighbour after neighbour, and its search skips keypoints of the current key frame that already hold a map point
    (ORBmatcher.cc:700-704): a point created for neighbour k fills a slot of the current key frame that the search for neighbour k + 1 no longer visits.  The batched
    search sees every slot as it was on entry, so it may return a match for such a slot; the tail drops it (`the slot is filled`), and that is the whole difference,
    because in SearchForTriangulation the entries of the current key frame do not influence each other: vbMatched2 is never set there, and CreateNewMapPoints builds its
    matcher with checkOri = false (:215), so no rotation histogram couples them.  The match of every other slot is therefore what the reference's later search finds.
    A new point fills a slot of neighbour k alone, and no neighbour is searched twice, so has_mp2 of a later neighbour is as on entry.  The triangulation of a match
    reads nothing of another match, and the two point updates read the point's own observations and camera centres, which the loop does not move.  This is the replay
    argument sind_match_fuse documents; tests/test_mappoints_cpu.py compares with the literal loop."""
    cur = keyframes[kf_id]
    kept = neighbours_for_triangulation(matcher, kf_id, keyframes, nn)
    if not kept:
        return []
    Ow1 = camera_centre(cur); k1 = _search_side(cur)
    step = max(1, int(getattr(matcher, "max_batch", len(kept))))         # one call each where the handle's max_batch holds the neighbours, else as few as it allows
    pairs = [(np.asarray(keyframes[k]["Tcw"], np.float32), Ow1, compute_f12(cur, keyframes[k], matcher.K5), k1, _search_side(keyframes[k])) for k in kept]
    check_ori, matcher.checkOri = matcher.checkOri, False               # ORBmatcher matcher(0.6, false)
    try:
        found = [f for a in range(0, len(kept), step) for f in matcher.SearchForTriangulation(pairs[a:a + step], False)]
    finally:
        matcher.checkOri = check_ori
    side1 = _tri_side(cur)
    pairs = [dict(Tcw1=cur["Tcw"], Twc1=pose_inverse(cur), Tcw2=keyframes[k]["Tcw"], Twc2=pose_inverse(keyframes[k]), kf1=side1, kf2=_tri_side(keyframes[k]), match12=f[0]) for k, f in zip(kept, found)]
    res = [r for a in range(0, len(kept), step) for r in matcher.Triangulate(pairs[a:a + step])]
    new = []
    for k, f, r in zip(kept, found, res):
        for idx1 in np.nonzero(r["status"] == 0)[0].tolist():
            if cur["mp"][idx1] >= 0:                                    # filled for an earlier neighbour: the reference's search would have skipped it
                continue
            new.append(_add_new_point(kf_id, k, idx1, f[0][idx1], r["x3D"][idx1], keyframes, mappoints))
    update_map_points(matcher, new, keyframes, mappoints)
    return new


def map_points_item(ids, keyframes, mappoints, descriptor=True, normal=True):
    """the dict ORBmatcher.UpdateMapPoints takes for the points `ids` (none of them bad), with kfs = the ids of its key frames"""
    kfs = sorted({k for m in ids for k in mappoints[m]["obs"]})
    row = {k: i for i, k in enumerate(kfs)}
    obs_start, obs_kf, obs_bad, obs_octave, obs_desc, ref_obs = [0], [], [], [], [], []
    for m in ids:
        mp = mappoints[m]; order = sorted(mp["obs"])
        if order and mp.get("ref_kf") not in mp["obs"]:
            mp["ref_kf"] = order[0]                                     # EraseObservation moves mpRefKF to mObservations.begin() when its key frame goes (src/MapPoint.cc:128-129)
        for k in order:
            kf = keyframes[k]; slot = mp["obs"][k]
            obs_kf.append(row[k]); obs_bad.append(1 if kf.get("bad") else 0); obs_octave.append(int(kf["octave"][slot])); obs_desc.append(np.asarray(kf["desc"][slot], np.uint8))
        obs_start.append(len(obs_kf)); ref_obs.append(order.index(mp["ref_kf"]) if mp.get("ref_kf") in mp["obs"] else -1)
    n = len(ids)
    have = lambda key: all(mappoints[m].get(key) is not None for m in ids)
    item = dict(Ow=np.array([camera_centre(keyframes[k]) for k in kfs], np.float32).reshape(len(kfs), 3), x3Dw=np.array([mappoints[m]["x3Dw"] for m in ids], np.float32).reshape(n, 3),
                obs_start=np.array(obs_start, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_bad=np.array(obs_bad, np.uint8), obs_octave=np.array(obs_octave, np.int32),
                obs_desc=np.array(obs_desc, np.uint8).reshape(len(obs_kf), 32), ref_obs=np.array(ref_obs, np.int32), do_descriptor=descriptor, do_normal=normal, kfs=kfs)
    for key, shape in (("desc", (n, 32)), ("normal", (n, 3)), ("max_dist", (n,)), ("min_dist", (n,))):
        if n and have(key):
            item[key] = np.array([mappoints[m][key] for m in ids]).reshape(shape)
    return item


def update_map_points(matcher, ids, keyframes, mappoints, descriptor=True, normal=True):
    """ComputeDistinctiveDescriptors (descriptor) and UpdateNormalAndDepth (normal) of the points `ids`, in one call of matcher.UpdateMapPoints; bad points are left alone, as
    both functions return on mbBad.  Writes desc, normal, max_dist, min_dist of the points the reference writes.  -> the ids that were passed on"""
    ids = [m for m in dict.fromkeys(ids) if not mappoints[m].get("bad")]
    for a in range(0, len(ids), MAX_POINTS_PER_ITEM):
        part = ids[a:a + MAX_POINTS_PER_ITEM]
        r = matcher.UpdateMapPoints([map_points_item(part, keyframes, mappoints, descriptor, normal)])[0]
        for j, m in enumerate(part):
            mp = mappoints[m]
            if descriptor and r["best_obs"][j] >= 0:
                mp["desc"] = np.array(r["desc"][j], np.uint8)
            if normal and r["updated"][j]:
                mp["normal"] = np.array(r["normal"][j], np.float32); mp["max_dist"] = np.float32(r["max_dist"][j]); mp["min_dist"] = np.float32(r["min_dist"][j])
    return ids


def process_new_keyframe_points(matcher, kf_id, keyframes, mappoints):
    """LocalMapping::ProcessNewKeyFrame, :139-161: every map point of the new key frame that is not bad and does not observe it yet gets AddObservation, UpdateNormalAndDepth
    and ComputeDistinctiveDescriptors; the others (new stereo points inserted by the tracking) are the recently added ones.  One update for all points: an update reads
    the point's own observations alone.  The map IS modified.  -> (updated ids, recently added ids)"""
    todo, recent = [], []
    for slot, m in enumerate(np.asarray(keyframes[kf_id]["mp"]).tolist()):
        if m < 0 or mappoints[m].get("bad"):
            continue
        if kf_id not in mappoints[m]["obs"]:
            mappoints[m]["obs"][kf_id] = slot; todo.append(m)
        else:
            recent.append(m)
    return update_map_points(matcher, todo, keyframes, mappoints), recent


def update_after_fuse(matcher, kf_id, keyframes, mappoints):
    """LocalMapping::SearchInNeighbors, :517-530: both updates for every map point of the current key frame that is not bad.  -> the updated ids"""
    return update_map_points(matcher, [m for m in np.asarray(keyframes[kf_id]["mp"]).tolist() if m >= 0], keyframes, mappoints)
