"""ORBmatcher — Python mirror of the reference's projection matchers of the RGB-D tracker (src/ORBmatcher.cc:45-129, :1328-1470, :1472-1599) over the C ABI."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib


class _Config(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("bounds", C.c_float * 4),
                ("scale_factors", C.c_float * 16), ("nlevels", C.c_int), ("cap_last", C.c_int), ("cap_cur", C.c_int), ("max_batch", C.c_int), ("device", C.c_int)]


class _Pair(C.Structure):
    _fields_ = [("Tcw_cur", C.c_void_p), ("Tcw_last", C.c_void_p),
                ("n_last", C.c_int), ("x3Dw", C.c_void_p), ("last_valid", C.c_void_p), ("last_has_obs", C.c_void_p), ("last_octave", C.c_void_p),
                ("last_angle", C.c_void_p), ("last_desc", C.c_void_p),
                ("n_cur", C.c_int), ("cur_un_xy", C.c_void_p), ("cur_octave", C.c_void_p), ("cur_angle", C.c_void_p), ("cur_u_right", C.c_void_p),
                ("cur_desc", C.c_void_p), ("grid_start", C.c_void_p), ("grid_idx", C.c_void_p), ("cur_taken", C.c_void_p),
                ("match_of_cur", C.c_void_p), ("nmatches", C.c_void_p)]


class _Local(C.Structure):
    _fields_ = [("Tcw", C.c_void_p),
                ("n_points", C.c_int), ("x3Dw", C.c_void_p), ("normal", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p), ("flags", C.c_void_p), ("desc", C.c_void_p),
                ("n_cur", C.c_int), ("cur_un_xy", C.c_void_p), ("cur_octave", C.c_void_p), ("cur_u_right", C.c_void_p), ("cur_desc", C.c_void_p),
                ("grid_start", C.c_void_p), ("grid_idx", C.c_void_p), ("cur_taken", C.c_void_p),
                ("in_view", C.c_void_p), ("proj_xyr", C.c_void_p), ("level", C.c_void_p), ("view_cos", C.c_void_p), ("n_to_match", C.c_void_p),
                ("match_of_cur", C.c_void_p), ("nmatches", C.c_void_p)]


class _Reloc(C.Structure):
    _fields_ = [("Tcw", C.c_void_p),
                ("n_points", C.c_int), ("x3Dw", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p), ("valid", C.c_void_p), ("kf_angle", C.c_void_p), ("desc", C.c_void_p),
                ("n_cur", C.c_int), ("cur_un_xy", C.c_void_p), ("cur_octave", C.c_void_p), ("cur_angle", C.c_void_p), ("cur_desc", C.c_void_p),
                ("grid_start", C.c_void_p), ("grid_idx", C.c_void_p), ("cur_taken", C.c_void_p),
                ("match_of_cur", C.c_void_p), ("nmatches", C.c_void_p)]


class _Bow(C.Structure):
    _fields_ = [("n_kf", C.c_int), ("kf_node", C.c_void_p), ("kf_valid", C.c_void_p), ("kf_angle", C.c_void_p), ("kf_desc", C.c_void_p),
                ("n_cur", C.c_int), ("cur_node", C.c_void_p), ("cur_angle", C.c_void_p), ("cur_desc", C.c_void_p),
                ("match_of_cur", C.c_void_p), ("nmatches", C.c_void_p)]


class _Tri(C.Structure):
    _fields_ = [("Tcw2", C.c_void_p), ("Cw1", C.c_void_p), ("F12", C.c_void_p),
                ("n1", C.c_int), ("node1", C.c_void_p), ("has_mp1", C.c_void_p), ("un_xy1", C.c_void_p), ("angle1", C.c_void_p), ("u_right1", C.c_void_p), ("desc1", C.c_void_p),
                ("n2", C.c_int), ("node2", C.c_void_p), ("has_mp2", C.c_void_p), ("un_xy2", C.c_void_p), ("octave2", C.c_void_p), ("angle2", C.c_void_p), ("u_right2", C.c_void_p),
                ("desc2", C.c_void_p), ("match12", C.c_void_p), ("nmatches", C.c_void_p)]


_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_u8 = lambda a: np.ascontiguousarray(a, np.uint8)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)


class ORBmatcher:
    """ORBmatcher(nnratio, checkOri) of the reference.  Provided: SearchByProjection(CurrentFrame, LastFrame, th, bMono) (TrackWithMotionModel),
    SearchLocalPoints = Frame::isInFrustum over the local map + SearchByProjection(F, vpMapPoints, th) (TrackLocalMap), and SearchByProjectionKF =
    SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (Relocalization).  A frame / a set of map points is a dict of arrays
    (see include/sind_hip.h: sind_match_pair, sind_match_local, sind_match_reloc).  By vocabulary node: SearchByBoW(pKF, F) (TrackReferenceKeyFrame, Relocalization;
    :159-288) and SearchForTriangulation (LocalMapping::CreateNewMapPoints; :657-823), on node ids from vocabulary.ORBVocabulary (sind_match_bow, sind_match_tri)."""
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, fx, fy, cx, cy, bf, bounds, scale_factors, nnratio=0.6, checkOri=True, cap=4096, max_batch=1, device=0, cap_points=0):
        cfg = _Config(fx, fy, cx, cy, bf, (C.c_float * 4)(*[float(b) for b in bounds]),
                      (C.c_float * 16)(*([float(s) for s in scale_factors] + [0.0] * (16 - len(scale_factors)))),
                      len(scale_factors), cap, cap, max_batch, device)
        self.checkOri, self.nnratio = checkOri, nnratio
        h = C.c_void_p()
        check(lib().sind_match_create(C.byref(cfg), C.byref(h)), "sind_match_create")
        self._h = h
        if cap_points:
            self.reserve_map_points(cap_points)

    def close(self):
        if getattr(self, "_h", None):
            lib().sind_match_destroy(self._h); self._h = None

    __del__ = close

    def SearchByProjection(self, pairs, th, bMono=False):
        """pairs: list of (Tcw_cur, Tcw_last, last, cur) -> list of (match_of_cur i32 [n_cur], nmatches)"""
        keep, arr = [], (_Pair * len(pairs))()
        f32 = lambda a: np.ascontiguousarray(a, np.float32); u8 = lambda a: np.ascontiguousarray(a, np.uint8); i32 = lambda a: np.ascontiguousarray(a, np.int32)
        outs = []
        for b, (tc, tl, last, cur) in enumerate(pairs):
            a = dict(Tcw_cur=f32(tc), Tcw_last=f32(tl), x3Dw=f32(last["x3Dw"]), last_valid=u8(last["valid"]), last_has_obs=u8(last["has_obs"]),
                     last_octave=i32(last["octave"]), last_angle=f32(last["angle"]), last_desc=u8(last["desc"]), cur_un_xy=f32(cur["un_xy"]),
                     cur_octave=i32(cur["octave"]), cur_angle=f32(cur["angle"]), cur_u_right=f32(cur["u_right"]), cur_desc=u8(cur["desc"]),
                     grid_start=i32(cur["grid_start"]), grid_idx=i32(cur["grid_idx"]))
            if cur.get("taken") is not None:
                a["cur_taken"] = u8(cur["taken"])
            nl, nc = len(a["last_valid"]), len(a["cur_octave"])
            a["match_of_cur"] = np.full(max(nc, 1), -1, np.int32); a["nmatches"] = np.zeros(1, np.int32)
            keep.append(a); arr[b].n_last = nl; arr[b].n_cur = nc
            for k, v in a.items():
                setattr(arr[b], k, v.ctypes.data if v.size else None)
            outs.append((a["match_of_cur"], a["nmatches"], nc))
        check(lib().sind_match_by_projection(self._h, arr, len(pairs), C.c_float(th), int(bMono), int(self.checkOri)), "sind_match_by_projection")
        return [(m[:nc].copy(), int(n[0])) for m, n, nc in outs]

    def reserve_map_points(self, cap_points):
        """capacity for local map points per frame; needed once before SearchLocalPoints (or pass cap_points to the constructor)"""
        check(lib().sind_match_reserve_map_points(self._h, int(cap_points)), "sind_match_reserve_map_points")

    def _call(self, fn, name, arr, keep, *args):
        for b, a in enumerate(keep):
            for k, v in a.items():
                setattr(arr[b], k, v.ctypes.data if v.size else None)
        check(fn(self._h, arr, len(keep), *args), name)

    def SearchLocalPoints(self, frames, th, viewingCosLimit=0.5):
        """frames: list of (Tcw, mp, cur); mp: x3Dw, normal, max_dist, min_dist, flags (bit0 candidate, bit1 observed), desc; cur as for SearchByProjection
        (angle unused).  Uses the constructor's nnratio.  -> list of dicts: match_of_cur i32 [n_cur] (index of the map point, -1: none), nmatches,
        in_view u8 [n], proj_xyr f32 [n, 3], level i32 [n], view_cos f32 [n], n_to_match."""
        keep, arr, outs = [], (_Local * len(frames))(), []
        for b, (T, mp, cur) in enumerate(frames):
            a = dict(Tcw=_f32(T), x3Dw=_f32(mp["x3Dw"]), normal=_f32(mp["normal"]), max_dist=_f32(mp["max_dist"]), min_dist=_f32(mp["min_dist"]), flags=_u8(mp["flags"]),
                     desc=_u8(mp["desc"]), cur_un_xy=_f32(cur["un_xy"]), cur_octave=_i32(cur["octave"]), cur_u_right=_f32(cur["u_right"]), cur_desc=_u8(cur["desc"]),
                     grid_start=_i32(cur["grid_start"]), grid_idx=_i32(cur["grid_idx"]))
            if cur.get("taken") is not None:
                a["cur_taken"] = _u8(cur["taken"])
            n, nc = len(a["flags"]), len(a["cur_octave"])
            a.update(in_view=np.zeros(max(n, 1), np.uint8), proj_xyr=np.zeros((max(n, 1), 3), np.float32), level=np.zeros(max(n, 1), np.int32), view_cos=np.zeros(max(n, 1), np.float32),
                     n_to_match=np.zeros(1, np.int32), match_of_cur=np.full(max(nc, 1), -1, np.int32), nmatches=np.zeros(1, np.int32))
            keep.append(a); arr[b].n_points = n; arr[b].n_cur = nc; outs.append((a, n, nc))
        self._call(lib().sind_match_local_map, "sind_match_local_map", arr, keep, C.c_float(th), C.c_float(self.nnratio), C.c_float(viewingCosLimit))
        return [dict(match_of_cur=a["match_of_cur"][:nc].copy(), nmatches=int(a["nmatches"][0]), in_view=a["in_view"][:n].copy(), proj_xyr=a["proj_xyr"][:n].copy(),
                     level=a["level"][:n].copy(), view_cos=a["view_cos"][:n].copy(), n_to_match=int(a["n_to_match"][0])) for a, n, nc in outs]

    def SearchByProjectionKF(self, pairs, th, ORBdist):
        """pairs: list of (Tcw_cur, kf, cur); kf, per slot of the key frame: x3Dw, max_dist, min_dist, valid (pMP && !isBad && not already found), angle, desc;
        cur as for SearchByProjection, taken = the keypoint holds any map point.  At most `cap` slots.  -> list of (match_of_cur i32 [n_cur], nmatches)"""
        keep, arr, outs = [], (_Reloc * len(pairs))(), []
        for b, (T, kf, cur) in enumerate(pairs):
            a = dict(Tcw=_f32(T), x3Dw=_f32(kf["x3Dw"]), max_dist=_f32(kf["max_dist"]), min_dist=_f32(kf["min_dist"]), valid=_u8(kf["valid"]), kf_angle=_f32(kf["angle"]),
                     desc=_u8(kf["desc"]), cur_un_xy=_f32(cur["un_xy"]), cur_octave=_i32(cur["octave"]), cur_angle=_f32(cur["angle"]), cur_desc=_u8(cur["desc"]),
                     grid_start=_i32(cur["grid_start"]), grid_idx=_i32(cur["grid_idx"]))
            if cur.get("taken") is not None:
                a["cur_taken"] = _u8(cur["taken"])
            n, nc = len(a["valid"]), len(a["cur_octave"])
            a.update(match_of_cur=np.full(max(nc, 1), -1, np.int32), nmatches=np.zeros(1, np.int32))
            keep.append(a); arr[b].n_points = n; arr[b].n_cur = nc; outs.append((a, nc))
        self._call(lib().sind_match_by_projection_kf, "sind_match_by_projection_kf", arr, keep, C.c_float(th), int(ORBdist), int(self.checkOri))
        return [(a["match_of_cur"][:nc].copy(), int(a["nmatches"][0])) for a, nc in outs]

    def SearchByBoW(self, pairs, nnratio=None):
        """pairs: list of (kf, cur); kf, per keypoint of the key frame: node (as ORBVocabulary.transform returns it), valid (pMP && !isBad), angle, desc (the key
        frame's own descriptors); cur: node, angle, desc.  nnratio None = the constructor's.  -> list of (match_of_cur i32 [n_cur], nmatches)"""
        keep, arr, outs = [], (_Bow * len(pairs))(), []
        for b, (kf, cur) in enumerate(pairs):
            a = dict(kf_node=_i32(kf["node"]), kf_valid=_u8(kf["valid"]), kf_angle=_f32(kf["angle"]), kf_desc=_u8(kf["desc"]),
                     cur_node=_i32(cur["node"]), cur_angle=_f32(cur["angle"]), cur_desc=_u8(cur["desc"]))
            n, nc = len(a["kf_node"]), len(a["cur_node"])
            a.update(match_of_cur=np.full(max(nc, 1), -1, np.int32), nmatches=np.zeros(1, np.int32))
            keep.append(a); arr[b].n_kf = n; arr[b].n_cur = nc; outs.append((a, nc))
        self._call(lib().sind_match_by_bow, "sind_match_by_bow", arr, keep, C.c_float(self.nnratio if nnratio is None else nnratio), int(self.checkOri))
        return [(a["match_of_cur"][:nc].copy(), int(a["nmatches"][0])) for a, nc in outs]

    def SearchForTriangulation(self, pairs, bOnlyStereo=False):
        """pairs: list of (Tcw2, Cw1, F12, kf1, kf2); kf1, per keypoint: node, has_mp, un_xy, angle, u_right, desc; kf2: the same and octave.
        -> list of (match12 i32 [n1], nmatches, matched_pairs i64 [nmatches, 2] = vMatchedPairs, ascending idx1)"""
        keep, arr, outs = [], (_Tri * len(pairs))(), []
        for b, (T2, Cw1, F12, k1, k2) in enumerate(pairs):
            a = dict(Tcw2=_f32(T2), Cw1=_f32(Cw1), F12=_f32(F12))
            for s, k in (("1", k1), ("2", k2)):
                a.update({"node" + s: _i32(k["node"]), "has_mp" + s: _u8(k["has_mp"]), "un_xy" + s: _f32(k["un_xy"]), "angle" + s: _f32(k["angle"]), "u_right" + s: _f32(k["u_right"]),
                          "desc" + s: _u8(k["desc"])})
            a["octave2"] = _i32(k2["octave"])
            n1, n2 = len(a["node1"]), len(a["node2"])
            a.update(match12=np.full(max(n1, 1), -1, np.int32), nmatches=np.zeros(1, np.int32))
            keep.append(a); arr[b].n1 = n1; arr[b].n2 = n2; outs.append((a, n1))
        self._call(lib().sind_match_for_triangulation, "sind_match_for_triangulation", arr, keep, int(bOnlyStereo), int(self.checkOri))
        res = []
        for a, n1 in outs:
            m = a["match12"][:n1].copy(); i1 = np.nonzero(m >= 0)[0]
            res.append((m, int(a["nmatches"][0]), np.stack([i1, m[i1]], 1).astype(np.int64)))
        return res

    def last_rounds(self):
        return lib().sind_match_last_rounds(self._h)
