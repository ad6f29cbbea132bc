"""The literal loops the covisibility table replaces, on plain Python containers: a dict model of the table's state, the counter of KeyFrame::UpdateConnections /
Tracking::UpdateLocalKeyFrames (src/KeyFrame.cc:302-320, src/Tracking.cc:1272-1288), the inner loop of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:651-691) with
its early break, and Tracking::UpdateLocalKeyFrames, LocalMapping::KeyFrameCulling and KeyFrame::SetBadFlag whole on the dict schema of sindslam_amd.covisibility.
Every walk copies the point's observation map first, as the reference does.  Pointer order is ascending id."""
import numpy as np


class Model:
    """the table as dicts: cells {(kf, idx): (point, octave, stereo)}; observations, nObs and the octave histogram derived from them"""

    def __init__(self, nlevels):
        self.nlevels, self.cells = nlevels, {}

    def apply(self, ops):
        for kf, idx, point, octave, stereo in ops:
            if point < 0:
                self.cells.pop((kf, idx), None)
            else:
                self.cells[(kf, idx)] = (point, octave, int(bool(stereo)))

    def row(self, kf, cap_feat):
        point = np.full(cap_feat, -1, np.int32); octave = np.zeros(cap_feat, np.uint8); stereo = np.zeros(cap_feat, np.uint8)
        for (k, idx), (p, o, s) in self.cells.items():
            if k == kf:
                point[idx], octave[idx], stereo[idx] = p, o, s
        return point, octave, stereo

    def observations(self):
        """{point: {kf: idx}}: mObservations of every point (the first cell wins where a point sits twice in a row, which the contract rules out)"""
        obs = {}
        for (k, idx), (p, _, _) in sorted(self.cells.items()):
            obs.setdefault(p, {}).setdefault(k, idx)
        return obs

    def points(self, ids):
        n_obs = np.zeros(len(ids), np.int32); hist = np.zeros((len(ids), self.nlevels), np.int32); at = {int(p): i for i, p in enumerate(ids)}
        for (k, idx), (p, o, s) in self.cells.items():
            if p in at:
                n_obs[at[p]] += 2 if s else 1; hist[at[p], o] += 1
        return n_obs, hist

    def n_obs(self, point):
        return int(self.points([point])[0][0])


def count_literal(points, self_kf, obs, cap_kf):
    """KFcounter of :302-320 (self_kf: the mnId == mnId skip) and keyframeCounter of Tracking.cc:1272-1288 (self_kf = -1) as an array over key frames; a -1 entry is a
    NULL or bad point"""
    counter = {}
    for m in points:
        if m < 0:
            continue
        observations = dict(obs.get(int(m), {}))                       # map<KeyFrame*,size_t> observations = pMP->GetObservations();
        for k in sorted(observations):
            if k == self_kf:
                continue
            counter[k] = counter.get(k, 0) + 1
    out = np.zeros(cap_kf, np.int32)
    for k, c in counter.items():
        out[k] = c
    return out


def cull_literal(kf, points, octave, close, model, th_obs=3):
    """LocalMapping.cc:651-691 for one key frame on the model -> (nMPs, nRedundantObservations, redundant per entry)"""
    obs = model.observations(); n_mps = n_red = 0; flags = np.zeros(len(points), np.uint8)
    for i, m in enumerate(points):
        if m < 0:                                                      # if(pMP) if(!pMP->isBad())
            continue
        if not close[i]:                                               # mvDepth[i] > mThDepth || mvDepth[i] < 0: continue
            continue
        n_mps += 1
        if model.n_obs(int(m)) > th_obs:
            scale_level = int(octave[i])
            observations = dict(obs.get(int(m), {}))
            n = 0
            for k in sorted(observations):
                if k == kf:
                    continue
                scale_level_i = model.cells[(k, observations[k])][1]
                if scale_level_i <= scale_level + 1:
                    n += 1
                    if n >= th_obs:
                        break
            if n >= th_obs:
                n_red += 1; flags[i] = 1
    return n_mps, n_red, flags


# ---- the dict schema ----
def n_obs(m, keyframes, mappoints):
    return sum(2 if keyframes[k]["u_right"][idx] >= 0 else 1 for k, idx in mappoints[m]["obs"].items())


def update_local_keyframes(frame_mp, keyframes, mappoints, frame_id):
    """Tracking::UpdateLocalKeyFrames (:1268-1376) -> (mvpLocalKeyFrames, mpReferenceKF), (None, None) on the early return"""
    counter = {}
    for i in range(len(frame_mp)):
        if frame_mp[i] >= 0:
            m = int(frame_mp[i])
            if not mappoints[m].get("bad"):
                observations = dict(mappoints[m]["obs"])
                for k in sorted(observations):
                    counter[k] = counter.get(k, 0) + 1
            else:
                frame_mp[i] = -1
    if not counter:
        return None, None
    best, kf_max, local = 0, None, []
    for k in sorted(counter):
        if keyframes[k].get("bad"):
            continue
        if counter[k] > best:
            best, kf_max = counter[k], k
        local.append(k)
        keyframes[k]["track_ref_frame"] = frame_id
    it_end = len(local)
    for it in range(it_end):
        if len(local) > 80:
            break
        kf = keyframes[local[it]]
        for q in list(kf.get("covisible", []))[:10]:
            if not keyframes[q].get("bad"):
                if keyframes[q].get("track_ref_frame") != frame_id:
                    local.append(q); keyframes[q]["track_ref_frame"] = frame_id
                    break
        for q in sorted(kf.get("children", set())):
            if not keyframes[q].get("bad"):
                if keyframes[q].get("track_ref_frame") != frame_id:
                    local.append(q); keyframes[q]["track_ref_frame"] = frame_id
                    break
        parent = kf.get("parent")
        if parent is not None:
            if keyframes[parent].get("track_ref_frame") != frame_id:
                local.append(parent); keyframes[parent]["track_ref_frame"] = frame_id
                break
    return local, kf_max


def update_best_covisibles(kf):
    w = kf["weights"]
    kf["covisible"] = sorted(w, key=lambda r: (-w[r], r))


def map_point_set_bad_flag(m, keyframes, mappoints):
    """MapPoint::SetBadFlag (src/MapPoint.cc:151-168)"""
    p = mappoints[m]
    p["bad"] = True
    obs = dict(p["obs"]); p["obs"] = {}
    for k in sorted(obs):
        keyframes[k]["mp"][obs[k]] = -1                               # pKF->EraseMapPointMatch(mit->second)


def erase_observation(m, k, keyframes, mappoints):
    """MapPoint::EraseObservation (:111-137); nObs is kept as the sum over the observations"""
    p = mappoints[m]; bad = False
    if k in p["obs"]:
        del p["obs"][k]
        if p.get("ref_kf") == k and p["obs"]:
            p["ref_kf"] = min(p["obs"])
        if n_obs(m, keyframes, mappoints) <= 2:
            bad = True
    if bad:
        map_point_set_bad_flag(m, keyframes, mappoints)


def set_bad_flag(k, keyframes, mappoints):
    """KeyFrame::SetBadFlag (src/KeyFrame.cc:453-545)"""
    kf = keyframes[k]
    if k == 0:
        return
    elif kf.get("not_erase"):
        kf["to_be_erased"] = True
        return
    for q in sorted(kf.get("weights", {})):
        other = keyframes[q]                                           # EraseConnection
        if k in other.get("weights", {}):
            del other["weights"][k]
            update_best_covisibles(other)
    mp = kf["mp"]
    for i in range(len(mp)):
        if mp[i] >= 0:
            erase_observation(int(mp[i]), k, keyframes, mappoints)
    kf["weights"] = {}; kf["covisible"] = []
    parent = kf.get("parent"); children = kf.setdefault("children", set())
    candidates = set()
    if parent is not None:
        candidates.add(parent)
    while children:
        go_on = False; best = -1; pc = pp = None
        for c in sorted(children):
            child = keyframes[c]
            if child.get("bad"):
                continue
            for q in child.get("covisible", []):
                for cand in sorted(candidates):
                    if q == cand:
                        w = child.get("weights", {}).get(q, 0)
                        if w > best:
                            pc, pp, best, go_on = c, q, w, True
        if go_on:
            keyframes[pc]["parent"] = pp; keyframes[pp].setdefault("children", set()).add(pc)
            candidates.add(pc); children.remove(pc)
        else:
            break
    if parent is not None:
        for c in sorted(children):
            keyframes[c]["parent"] = parent; keyframes[parent].setdefault("children", set()).add(c)
        keyframes[parent].setdefault("children", set()).discard(k)
    kf["bad"] = True


def keyframe_culling(cur, keyframes, mappoints, th_depth):
    """LocalMapping::KeyFrameCulling (:632-696) -> the key frames for which SetBadFlag erased something, in order"""
    erased = []
    local = list(keyframes[cur].get("covisible", []))
    for k in local:
        if k == 0:
            continue
        kf = keyframes[k]
        mp = list(np.asarray(kf["mp"]).tolist())
        th_obs = 3; n_red = 0; n_mps = 0
        for i in range(len(mp)):
            m = mp[i]
            if m >= 0:
                if not mappoints[m].get("bad"):
                    if th_depth is not None:
                        if kf["depth"][i] > th_depth or kf["depth"][i] < 0:
                            continue
                    n_mps += 1
                    if n_obs(m, keyframes, mappoints) > th_obs:
                        scale_level = int(kf["octave"][i])
                        observations = dict(mappoints[m]["obs"])
                        n = 0
                        for ki in sorted(observations):
                            if ki == k:
                                continue
                            scale_level_i = int(keyframes[ki]["octave"][observations[ki]])
                            if scale_level_i <= scale_level + 1:
                                n += 1
                                if n >= th_obs:
                                    break
                        if n >= th_obs:
                            n_red += 1
        if n_red > 0.9 * n_mps:
            was = bool(kf.get("bad"))
            set_bad_flag(k, keyframes, mappoints)
            if kf.get("bad") and not was:
                erased.append(k)
    return erased
