"""The covisibility graph over the C ABI (include/sind_hip.h: sind_covis_*): the observations of the map live in a device-resident table, and the three walks the
reference makes over MapPoint::mObservations -- KeyFrame::UpdateConnections (src/KeyFrame.cc:289-379), Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1268-1380) and
LocalMapping::KeyFrameCulling (src/LocalMapping.cc:632-696) -- become a query that uploads a list of point ids, with the order-dependent tails here on the host.

The map is the dict schema of optimizer.py and mapping.py.  Key frames {id: dict(mp i64 [n] (-1: none), octave [n], u_right [n], depth [n], bad, parent (id or None),
children (set of ids), weights {id: shared points}, covisible (ids, most shared points first), not_erase / to_be_erased (optional flags), track_ref_frame (written
here: mnTrackReferenceForFrame))}; map points {id: dict(obs {kf id: idx}, bad, ref_kf (optional))}.  Key-frame ids are rows of the table and point ids its points.
Where the reference walks a container keyed by pointers this walks ascending ids: unpinned, as elsewhere."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import SindError, lib

TH_OBS = 3                                                             # thObs of KeyFrameCulling (LocalMapping.cc:647-648)


class _Op(C.Structure):
    _fields_ = [("kf", C.c_int), ("idx", C.c_int), ("point", C.c_int), ("octave", C.c_int), ("stereo", C.c_int)]


class _Query(C.Structure):
    _fields_ = [("self_kf", C.c_int), ("n", C.c_int), ("points", C.c_void_p), ("count", C.c_void_p)]


class _CullItem(C.Structure):
    _fields_ = [("kf", C.c_int), ("n", C.c_int), ("points", C.c_void_p), ("octave", C.c_void_p), ("close", C.c_void_p), ("n_mps", C.c_void_p), ("n_redundant", C.c_void_p),
                ("redundant", C.c_void_p)]


_host = None


def _host_lib():
    """libsind_host.so: the host twins sindh_covis_* (the same per-element source as the kernels, csrc/host/covis.hpp)"""
    global _host
    if _host is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsind_host.so")
        if not os.path.exists(path):
            raise SindError(f"{path} not built")
        _host = C.CDLL(path)
    return _host


def _p(a):
    return C.c_void_p(a.ctypes.data if a.size else None)


class CovisibilityTable:
    """cap_kf key frames of cap_feat features each, point ids below cap_points, nlevels pyramid levels; max_queries lists or cull items per launch (more are split into
    several calls).  host=True runs the host twin, which needs no device.  Ops are queued and go to the table in one apply: before a query, at flush(), or when a second op
    meets a cell that is already queued (a call may hold one op per cell)."""

    def __init__(self, cap_kf, cap_feat, cap_points, nlevels, host=False, max_queries=64, device=0):
        self.host = bool(host); self._L = _host_lib() if host else lib(); self._pre = "sindh_covis_" if host else "sind_covis_"
        self.cap_kf, self.cap_feat, self.cap_points, self.nlevels, self.max_queries = int(cap_kf), int(cap_feat), int(cap_points), int(nlevels), int(max_queries)
        self._h = None; h = C.c_void_p()
        self._check(self._fn("create")(self.cap_kf, self.cap_feat, self.cap_points, self.nlevels, self.max_queries, int(device), C.byref(h)), "create")
        self._h = h; self._ops = []; self._cells = set()

    def _fn(self, name):
        return getattr(self._L, self._pre + name)

    def _check(self, rc, what):
        if rc < 0:
            text = "" if self.host else ": " + lib().sind_last_error().decode(errors="replace")
            raise SindError(f"{self._pre}{what} failed ({rc}){text}")

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h); self._h = None

    __del__ = close

    # ---- updates ----
    def _queue(self, kf, idx, point, octave, stereo):
        cell = (int(kf), int(idx))
        if cell in self._cells:
            self.flush()
        self._cells.add(cell); self._ops.append((cell[0], cell[1], int(point), int(octave), int(bool(stereo))))

    def add_observation(self, kf, idx, point, octave, stereo):
        """MapPoint::AddObservation(pKF, idx): the cell takes the point (an occupied cell is replaced)"""
        self._queue(kf, idx, point, octave, stereo)

    def erase_observation(self, kf, idx):
        """MapPoint::EraseObservation(pKF) for the point in cell (kf, idx)"""
        self._queue(kf, idx, -1, 0, 0)

    def set_point_bad(self, obs):
        """MapPoint::SetBadFlag: obs = the point's observations {kf: idx} as they were; all its cells are cleared"""
        for k, idx in sorted(obs.items()):
            self.erase_observation(k, idx)

    def replace(self, old_obs, new, new_obs, keyframes):
        """MapPoint::Replace (src/MapPoint.cc:177-216): old_obs / new_obs = the observations of the two points BEFORE the call.  Where the new point is not in the key
        frame the old one's cell passes to it, elsewhere the cell is cleared."""
        for k, idx in sorted(old_obs.items()):
            if k not in new_obs:
                kf = keyframes[k]; self.add_observation(k, idx, new, kf["octave"][idx], kf["u_right"][idx] >= 0)
            else:
                self.erase_observation(k, idx)

    def erase_keyframe(self, kf):
        """every cell of the row cleared (the EraseObservation loop of KeyFrame::SetBadFlag, whatever the caller's mp says)"""
        point = self.read_row(kf)[0]
        for idx in np.nonzero(point >= 0)[0].tolist():
            self.erase_observation(kf, idx)

    def flush(self):
        if self._ops:
            arr = (_Op * len(self._ops))(*self._ops); n = len(self._ops)
            self._ops, self._cells = [], set()
            self._check(self._fn("apply")(self._h, arr, n), "apply")

    def clear(self):
        self._ops, self._cells = [], set()
        self._check(self._fn("clear")(self._h), "clear")

    def from_map(self, keyframes, mappoints):
        """the table of a map: cleared, then one cell per observation of every point -> self"""
        self.clear()
        for m in sorted(mappoints):
            for k, idx in sorted(mappoints[m]["obs"].items()):
                kf = keyframes[k]; self.add_observation(k, idx, m, kf["octave"][idx], kf["u_right"][idx] >= 0)
        self.flush()
        return self

    # ---- read-back ----
    def read_row(self, kf):
        """-> point i32, octave u8, stereo u8 [cap_feat]"""
        self.flush()
        point = np.empty(self.cap_feat, np.int32); octave = np.empty(self.cap_feat, np.uint8); stereo = np.empty(self.cap_feat, np.uint8)
        self._check(self._fn("read_row")(self._h, int(kf), _p(point), _p(octave), _p(stereo)), "read_row")
        return point, octave, stereo

    def read_points(self, points):
        """-> n_obs i32 [n], hist i32 [n][nlevels]"""
        self.flush()
        pts = np.ascontiguousarray(points, np.int32); n_obs = np.zeros(len(pts), np.int32); hist = np.zeros((len(pts), self.nlevels), np.int32)
        self._check(self._fn("read_points")(self._h, _p(pts), len(pts), _p(n_obs), _p(hist)), "read_points")
        return n_obs, hist

    # ---- queries ----
    def _batches(self, sizes):
        """consecutive runs of at most max_queries items whose sizes add up to at most 64 * ceil(max_queries / 64) (the tag bits a count call may use)"""
        room = 64 * ((self.max_queries + 63) // 64); out, cur, used = [], [], 0
        for j, s in enumerate(sizes):
            if cur and (len(cur) == self.max_queries or used + s > room):
                out.append(cur); cur, used = [], 0
            cur.append(j); used += s
        if cur:
            out.append(cur)
        return out

    def count(self, lists, self_kfs):
        """lists of point ids (-1: skipped), one self_kf each (-1: none) -> count i32 [cap_kf] per list"""
        self.flush()
        pts = [np.ascontiguousarray(l, np.int32) for l in lists]; out = [np.zeros(self.cap_kf, np.int32) for _ in pts]
        mult = [int(np.unique(p[p >= 0], return_counts=True)[1].max(initial=0)) for p in pts]
        for batch in ([list(range(len(pts)))] if self.host else self._batches(mult)):
            arr = (_Query * len(batch))()
            for q, j in zip(arr, batch):
                q.self_kf, q.n, q.points, q.count = int(self_kfs[j]), len(pts[j]), _p(pts[j]), _p(out[j])
            self._check(self._fn("count")(self._h, arr, len(batch)), "count")
        return out

    def cull(self, items, th_obs=TH_OBS):
        """items: (kf, points, octave, close) -> (n_mps, n_redundant, redundant u8 [n]) per item"""
        self.flush()
        keep = [(int(k), np.ascontiguousarray(p, np.int32), np.ascontiguousarray(o, np.uint8), np.ascontiguousarray(c, np.uint8)) for k, p, o, c in items]
        res = [(np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(len(p), np.uint8)) for _, p, _, _ in keep]
        for batch in ([list(range(len(keep)))] if self.host else self._batches([0] * len(keep))):
            arr = (_CullItem * len(batch))()
            for it, j in zip(arr, batch):
                k, p, o, c = keep[j]
                if not len(p) == len(o) == len(c):
                    raise ValueError("CovisibilityTable.cull: points, octave and close of different lengths")
                it.kf, it.n, it.points, it.octave, it.close = k, len(p), _p(p), _p(o), _p(c)
                it.n_mps, it.n_redundant, it.redundant = _p(res[j][0]), _p(res[j][1]), _p(res[j][2])
            self._check(self._fn("cull")(self._h, arr, len(batch), int(th_obs)), "cull")
        return [(int(a[0]), int(b[0]), r) for a, b, r in res]


def good_points(mp, mappoints):
    """a key frame's or frame's mvpMapPoints as a query list: NULL and isBad() points become -1"""
    return np.array([m if m >= 0 and not mappoints[m].get("bad") else -1 for m in np.asarray(mp).tolist()], np.int32)


def update_connections_many(table, ks, keyframes, mappoints):
    """KeyFrame::UpdateConnections for every key frame of ks, in that order: ONE count call for all of them, then the tail (:322-378) of each in order on the host.
    Leaves the dicts exactly as successive optimizer.update_connections(k, keyframes, mappoints) calls do.  The batch equals the sequence because UpdateConnections
    READS only observations and bad flags of points (:302-320) and WRITES only weights and ordered lists of key frames: no call changes what a later call counts, so
    the counts taken up front are the counts each call would have taken in its turn; the tails, which do read what earlier tails wrote (AddConnection re-sorts the
    other side over all of its weights), run here in order.  Ties are broken by ascending id, as in that function; the first-connection parent stays the map
    builder's, as there."""
    ks = list(ks)
    counts = table.count([good_points(keyframes[k]["mp"], mappoints) for k in ks], ks)
    for k, cnt in zip(ks, counts):
        counter = {int(q): int(cnt[q]) for q in np.nonzero(cnt)[0]}
        if not counter:
            continue
        best = max(sorted(counter), key=lambda q: counter[q])
        near = [q for q in counter if counter[q] >= 15] or [best]
        for q in near:
            o = keyframes[q]; o.setdefault("weights", {})[k] = counter[q]
            o["covisible"] = sorted(o["weights"], key=lambda r: (-o["weights"][r], r))
        kf = keyframes[k]
        kf["weights"] = dict(counter)
        kf["covisible"] = sorted(near, key=lambda q: (-counter[q], q))


def update_local_keyframes(table, frame_mp, keyframes, mappoints, frame_id):
    """Tracking::UpdateLocalKeyFrames (:1268-1376).  frame_mp: mCurrentFrame.mvpMapPoints as ids (-1: NULL); the entries of bad points are set to -1 in place
    (:1285); on the device it may hold cap_feat entries.  The vote (:1271-1288) is one count call with self_kf = -1; :1290-1375 follow literally: the voted key frames in ascending id (the reference: pointer
    order), then for each of THOSE one best-covisibility neighbour, one child and the parent, as far as not yet included -- the `break` after a parent is added is in
    the body of the outer loop and ends it (:1365), and nothing is added once there are more than 80 (:1322).  mnTrackReferenceForFrame is keyframes[k]["track_ref_frame"].
    -> (mvpLocalKeyFrames in order, mpReferenceKF); (None, None) where the reference returns early on an empty vote and leaves both as they were; the reference key frame
    is None where it is left as it was (every voted key frame bad)."""
    frame_mp = np.asarray(frame_mp)
    for i, m in enumerate(frame_mp.tolist()):
        if m >= 0 and mappoints[m].get("bad"):
            frame_mp[i] = -1
    cnt = table.count([frame_mp.astype(np.int32)], [-1])[0]
    counter = {int(k): int(cnt[k]) for k in np.nonzero(cnt)[0]}
    if not counter:
        return None, None
    best, kf_max, local = 0, None, []
    for k in sorted(counter):
        if keyframes[k].get("bad"):
            continue
        if counter[k] > best:
            best, kf_max = counter[k], k
        local.append(k); keyframes[k]["track_ref_frame"] = frame_id

    def take(k):
        if keyframes[k].get("track_ref_frame") != frame_id:
            local.append(k); keyframes[k]["track_ref_frame"] = frame_id
            return True
        return False

    for k in list(local):                                              # itEndKF is taken before the loop: the voted key frames alone
        if len(local) > 80:
            break
        kf = keyframes[k]
        for q in list(kf.get("covisible", ()))[:10]:                   # GetBestCovisibilityKeyFrames(10)
            if not keyframes[q].get("bad") and take(q):
                break
        for q in sorted(kf.get("children", ())):
            if not keyframes[q].get("bad") and take(q):
                break
        parent = kf.get("parent")
        if parent is not None and take(parent):
            break
    return local, kf_max


def _n_obs(obs, keyframes):
    """nObs of a point from its observations: 2 for a stereo keypoint (MapPoint.cc:105-108)"""
    return sum(2 if keyframes[k]["u_right"][idx] >= 0 else 1 for k, idx in obs.items())


def _erase_connection(kf, k):
    """KeyFrame::EraseConnection (:553-567) with UpdateBestCovisibles (:138-157)"""
    w = kf.get("weights", {})
    if k in w:
        del w[k]
        kf["covisible"] = sorted(w, key=lambda r: (-w[r], r))


def set_bad_flag(table, k, keyframes, mappoints):
    """KeyFrame::SetBadFlag (:453-545) on the dicts and the table.  Key frame 0 is never erased; a key frame with not_erase set gets to_be_erased and stays (:457-463).
    Otherwise: EraseConnection on every connected key frame; EraseObservation on every point of mp (the point loses its cell; at nObs <= 2 it goes bad,
    MapPoint::SetBadFlag: its observations are cleared and the mp entry of every key frame that held it becomes -1); the children are re-parented (the child with the
    heaviest link to a parent candidate first, the rest to this key frame's parent); the key frame leaves its parent's children and is bad.  -> True if it was erased"""
    kf = keyframes[k]
    if k == 0:
        return False
    if kf.get("not_erase"):
        kf["to_be_erased"] = True
        return False
    for q in sorted(kf.get("weights", {})):
        _erase_connection(keyframes[q], k)
    for m in np.asarray(kf["mp"]).tolist():
        if m < 0:
            continue
        p = mappoints[m]
        if k not in p["obs"]:
            continue
        table.erase_observation(k, p["obs"][k]); del p["obs"][k]
        if p.get("ref_kf") == k and p["obs"]:
            p["ref_kf"] = min(p["obs"])
        if _n_obs(p["obs"], keyframes) <= 2:
            obs = p["obs"]; p["obs"] = {}; p["bad"] = True
            table.set_point_bad(obs)
            for q, idx in sorted(obs.items()):
                keyframes[q]["mp"][idx] = -1
    kf["weights"] = {}; kf["covisible"] = []
    parent = kf.get("parent"); children = kf.setdefault("children", set())
    candidates = set() if parent is None else {parent}
    while children:
        best, pair = -1, None
        for c in sorted(children):
            child = keyframes[c]
            if child.get("bad"):
                continue
            for q in child.get("covisible", ()):
                if q in candidates:
                    w = child.get("weights", {}).get(q, 0)
                    if w > best:
                        best, pair = w, (c, q)
        if pair is None:
            break
        c, q = pair
        keyframes[c]["parent"] = q; keyframes[q].setdefault("children", set()).add(c)
        candidates.add(c); children.discard(c)
    if parent is not None:
        for c in sorted(children):
            keyframes[c]["parent"] = parent; keyframes[parent].setdefault("children", set()).add(c)
        keyframes[parent].setdefault("children", set()).discard(k)
    kf["bad"] = True
    return True


def cull_item(k, keyframes, mappoints, th_depth):
    """one key frame as a cull item: its points (NULL and bad: -1), octaves, and close[i] = not (mvDepth[i] > mThDepth or mvDepth[i] < 0) (:660; th_depth None:
    monocular, every entry counts)"""
    kf = keyframes[k]; depth = np.asarray(kf["depth"])
    close = np.ones(len(kf["mp"]), np.uint8) if th_depth is None else (~((depth > th_depth) | (depth < 0))).astype(np.uint8)
    return k, good_points(kf["mp"], mappoints), np.asarray(kf["octave"]).astype(np.uint8), close


def keyframe_culling(table, cur, keyframes, mappoints, th_depth, replay=True):
    """LocalMapping::KeyFrameCulling (:632-696) for the key frame cur.  -> the key frames erased, in order.
    The loop walks cur's covisible list as it was on entry (:638 copies it) and a key frame is erased where nRedundantObservations > 0.9 * nMPs (:693, FP64).  Erasing one
    changes n_obs of its points and may make points bad, so the verdict of a LATER key frame can depend on an earlier cull: one cull call over the whole list is exact
    only up to its first cull.  Replay: run the batch over the rest of the list, take the FIRST key frame that meets :693, apply set_bad_flag to the dicts and the
    table, run what follows it again: one launch per cull plus one.
    Why this equals the literal loop: the verdict of a key frame is a function of the map as it is when the loop reaches it, and the map changes only inside
    SetBadFlag.  Up to and including the first key frame with a positive verdict, the literal loop has changed nothing, so the batch -- evaluated on that same
    map -- gives each of them the literal loop's verdict; the first positive one is therefore the first the literal loop erases.  After set_bad_flag the map is the
    literal loop's map at that point, and the argument repeats on the rest.  A SetBadFlag that erases nothing (key frame 0 is skipped before; not_erase) changes
    nothing, so the batch stays valid and the scan goes on in it.
    replay=False evaluates ONE batch and erases every key frame it flags (what the batch alone would give; the tests use it to show that the replay matters)."""
    order = [k for k in list(keyframes[cur].get("covisible", ())) if k != 0]      # :643
    erased, pos = [], 0
    while pos < len(order):
        res = table.cull([cull_item(k, keyframes, mappoints, th_depth) for k in order[pos:]])
        again = False
        for j, (n_mps, n_red, _) in enumerate(res):
            was_bad = bool(keyframes[order[pos + j]].get("bad"))
            if n_red > 0.9 * n_mps and set_bad_flag(table, order[pos + j], keyframes, mappoints):
                if not was_bad:
                    erased.append(order[pos + j])
                if replay:
                    pos += j + 1; again = True
                    break
        if not again:
            break
    return erased
