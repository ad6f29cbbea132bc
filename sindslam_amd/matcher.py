"""ORBmatcher — Python mirror of the reference's projection matchers of the RGB-D tracker (src/ORBmatcher.cc:45-129, :1328-1470, :1472-1599), its vocabulary-guided
searches and its projections into a key frame (Fuse, SearchByProjection(pKF, Scw), SearchBySim3; :290-403, :825-1326) over the C ABI."""
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


class _BowKF(C.Structure):
    _fields_ = [("n1", C.c_int), ("node1", C.c_void_p), ("valid1", C.c_void_p), ("angle1", C.c_void_p), ("desc1", C.c_void_p),
                ("n2", C.c_int), ("node2", C.c_void_p), ("valid2", C.c_void_p), ("angle2", C.c_void_p), ("desc2", C.c_void_p),
                ("match12", C.c_void_p), ("nmatches", C.c_void_p)]


class _Tri(C.Structure):
    _fields_ = [("Tcw2", C.c_void_p), ("Cw1", C.c_void_p), ("F12", C.c_void_p),
                ("n1", C.c_int), ("node1", C.c_void_p), ("has_mp1", C.c_void_p), ("un_xy1", C.c_void_p), ("angle1", C.c_void_p), ("u_right1", C.c_void_p), ("desc1", C.c_void_p),
                ("n2", C.c_int), ("node2", C.c_void_p), ("has_mp2", C.c_void_p), ("un_xy2", C.c_void_p), ("octave2", C.c_void_p), ("angle2", C.c_void_p), ("u_right2", C.c_void_p),
                ("desc2", C.c_void_p), ("match12", C.c_void_p), ("nmatches", C.c_void_p)]


_POINTS = [("n_points", C.c_int), ("x3Dw", C.c_void_p), ("normal", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p), ("valid", C.c_void_p), ("desc", C.c_void_p)]


class _Fuse(C.Structure):
    _fields_ = [("Tcw", C.c_void_p)] + _POINTS + [("n_kf", C.c_int), ("kf_un_xy", C.c_void_p), ("kf_octave", C.c_void_p), ("kf_u_right", C.c_void_p), ("kf_desc", C.c_void_p),
                                                  ("grid_start", C.c_void_p), ("grid_idx", C.c_void_p), ("best_idx", C.c_void_p), ("best_dist", C.c_void_p), ("nfused", C.c_void_p)]


class _ProjSim3(C.Structure):
    _fields_ = [("Scw", C.c_void_p)] + _POINTS + [("n_kf", C.c_int), ("kf_un_xy", C.c_void_p), ("kf_octave", C.c_void_p), ("kf_desc", C.c_void_p), ("grid_start", C.c_void_p),
                                                  ("grid_idx", C.c_void_p), ("kf_taken", C.c_void_p), ("match_of_kf", C.c_void_p), ("nmatches", C.c_void_p)]


class _Sim3Side(C.Structure):
    _fields_ = [("n", C.c_int), ("valid", C.c_void_p), ("x3Dw", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p), ("mp_desc", C.c_void_p),
                ("un_xy", C.c_void_p), ("octave", C.c_void_p), ("kf_desc", C.c_void_p), ("grid_start", C.c_void_p), ("grid_idx", C.c_void_p)]


class _Sim3Pair(C.Structure):
    _fields_ = [("T1w", C.c_void_p), ("T2w", C.c_void_p), ("s12", C.c_float), ("R12", C.c_void_p), ("t12", C.c_void_p), ("side1", _Sim3Side), ("side2", _Sim3Side),
                ("match12", C.c_void_p), ("nfound", C.c_void_p)]


class _Sim3Item(C.Structure):
    _fields_ = [("T1w", C.c_void_p), ("T2w", C.c_void_p), ("n", C.c_int), ("x3Dw1", C.c_void_p), ("x3Dw2", C.c_void_p), ("sigma2_1", C.c_void_p), ("sigma2_2", C.c_void_p),
                ("n_its", C.c_int), ("triple", C.c_void_p), ("count", C.c_void_p), ("inlier_bits", C.c_void_p), ("s12", C.c_void_p), ("R12", C.c_void_p), ("t12", C.c_void_p)]


class _PnpItem(C.Structure):
    _fields_ = [("n", C.c_int), ("x3Dw", C.c_void_p), ("p2d", C.c_void_p), ("sigma2", C.c_void_p), ("th2", C.c_float), ("min_inliers", C.c_int), ("n_its", C.c_int), ("samples", C.c_void_p),
                ("best_count", C.c_int), ("best_bits", C.c_void_p), ("count", C.c_void_p), ("inlier_bits", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p), ("refine", C.c_void_p),
                ("n_refines", C.c_void_p), ("refine_hyp", C.c_void_p), ("refine_count", C.c_void_p), ("refine_bits", C.c_void_p), ("refine_R", C.c_void_p), ("refine_t", C.c_void_p)]


class _PoseOptItem(C.Structure):
    _fields_ = [("n", C.c_int), ("x3Dw", C.c_void_p), ("obs_xy", C.c_void_p), ("u_right", C.c_void_p), ("inv_sigma2", C.c_void_p), ("Tcw", C.c_void_p), ("Tcw_out", C.c_void_p),
                ("outlier", C.c_void_p), ("n_good", C.c_void_p), ("n_rounds", C.c_void_p), ("round_iters", C.c_void_p), ("round_nbad", C.c_void_p), ("round_pose", C.c_void_p),
                ("round_chi2", C.c_void_p), ("round_lambda", C.c_void_p)]


class _Sim3OptItem(C.Structure):
    _fields_ = [("n", C.c_int), ("s12", C.c_float), ("x3Dc1", C.c_void_p), ("x3Dc2", C.c_void_p), ("obs1_xy", C.c_void_p), ("obs2_xy", C.c_void_p), ("inv_sigma2_1", C.c_void_p),
                ("inv_sigma2_2", C.c_void_p), ("K1", C.c_void_p), ("K2", C.c_void_p), ("R12", C.c_void_p), ("t12", C.c_void_p), ("q_out", C.c_void_p), ("t_out", C.c_void_p),
                ("s_out", C.c_void_p), ("removed", C.c_void_p), ("n_inliers", C.c_void_p), ("n_bad", C.c_void_p), ("n_stages", C.c_void_p), ("stage_iters", C.c_void_p),
                ("stage_chi2", C.c_void_p), ("stage_lambda", C.c_void_p)]


class _LocalBaItem(C.Structure):
    _fields_ = [("n_kf", C.c_int), ("kf_id", C.c_void_p), ("kf_kind", C.c_void_p), ("Tcw", C.c_void_p), ("n_mp", C.c_int), ("mp_id", C.c_void_p), ("x3Dw", C.c_void_p),
                ("obs_start", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_xy", C.c_void_p), ("u_right", C.c_void_p), ("inv_sigma2", C.c_void_p), ("do_more", C.c_int),
                ("Tcw_out", C.c_void_p), ("x3Dw_out", C.c_void_p), ("erase", C.c_void_p), ("n_stages", C.c_void_p), ("stage_iters", C.c_void_p), ("n_level1", C.c_void_p),
                ("stage_chi2", C.c_void_p), ("stage_lambda", C.c_void_p)]


class _EssGraphItem(C.Structure):
    _fields_ = [("n_kf", C.c_int), ("kf_id", C.c_void_p), ("Tcw", C.c_void_p), ("has_corrected", C.c_void_p), ("corrected", C.c_void_p), ("has_noncorrected", C.c_void_p),
                ("noncorrected", C.c_void_p), ("fixed_kf", C.c_int), ("n_edges", C.c_int), ("edge_i", C.c_void_p), ("edge_j", C.c_void_p), ("edge_kind", C.c_void_p),
                ("n_mp", C.c_int), ("x3Dw", C.c_void_p), ("mp_ref", C.c_void_p), ("Siw_out", C.c_void_p), ("Tiw_out", C.c_void_p), ("x3Dw_out", C.c_void_p),
                ("n_iters", C.c_void_p), ("chi2", C.c_void_p), ("lambda_", C.c_void_p), ("n_active", C.c_void_p), ("solver_fail", C.c_void_p)]


class _GlobalBaItem(C.Structure):
    _fields_ = [("n_kf", C.c_int), ("kf_id", C.c_void_p), ("Tcw", C.c_void_p), ("n_mp", C.c_int), ("mp_id", C.c_void_p), ("x3Dw", C.c_void_p),
                ("obs_start", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_xy", C.c_void_p), ("u_right", C.c_void_p), ("inv_sigma2", C.c_void_p),
                ("Tcw_out", C.c_void_p), ("x3Dw_out", C.c_void_p), ("included", C.c_void_p), ("n_iters", C.c_void_p), ("chi2", C.c_void_p), ("lambda_", C.c_void_p),
                ("n_active_poses", C.c_void_p), ("solver_fail", C.c_void_p), ("env_entries", C.c_void_p), ("env_dense_entries", C.c_void_p)]


class _TriSide(C.Structure):
    _fields_ = [("n", C.c_int), ("xy", C.c_void_p), ("un_xy", C.c_void_p), ("octave", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p)]


class _TriPair(C.Structure):
    _fields_ = [("Tcw1", C.c_void_p), ("Twc1", C.c_void_p), ("Tcw2", C.c_void_p), ("Twc2", C.c_void_p), ("kf1", _TriSide), ("kf2", _TriSide), ("match12", C.c_void_p),
                ("x3D", C.c_void_p), ("how", C.c_void_p), ("status", C.c_void_p), ("nnew", C.c_void_p)]


class _MapPointsItem(C.Structure):
    _fields_ = [("n_kf", C.c_int), ("Ow", C.c_void_p), ("n_mp", C.c_int), ("x3Dw", C.c_void_p), ("obs_start", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_bad", C.c_void_p),
                ("obs_octave", C.c_void_p), ("obs_desc", C.c_void_p), ("ref_obs", C.c_void_p), ("do_descriptor", C.c_int), ("do_normal", C.c_int), ("desc_out", C.c_void_p),
                ("best_obs", C.c_void_p), ("normal_out", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p), ("updated", C.c_void_p)]


_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_u8 = lambda a: np.ascontiguousarray(a, np.uint8)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)


def _cur(cur, *floats):
    """the searched frame's fields of sind_match_pair / _local / _reloc, with the float arrays that the call reads besides un_xy"""
    a = dict(n_cur=len(cur["octave"]), cur_un_xy=_f32(cur["un_xy"]), cur_octave=_i32(cur["octave"]), cur_desc=_u8(cur["desc"]), grid_start=_i32(cur["grid_start"]), grid_idx=_i32(cur["grid_idx"]))
    a.update({"cur_" + k: _f32(cur[k]) for k in floats})
    if cur.get("taken") is not None:
        a["cur_taken"] = _u8(cur["taken"])
    return a


def _points_kf(mp, kf, u_right=False):
    """the map-point list and the key frame of sind_match_fuse_item / sind_match_proj_sim3"""
    a = dict(n_points=len(mp["valid"]), x3Dw=_f32(mp["x3Dw"]), normal=_f32(mp["normal"]), max_dist=_f32(mp["max_dist"]), min_dist=_f32(mp["min_dist"]), valid=_u8(mp["valid"]), desc=_u8(mp["desc"]),
             n_kf=len(kf["octave"]), kf_un_xy=_f32(kf["un_xy"]), kf_octave=_i32(kf["octave"]), kf_desc=_u8(kf["desc"]), grid_start=_i32(kf["grid_start"]), grid_idx=_i32(kf["grid_idx"]))
    if u_right:
        a["kf_u_right"] = _f32(kf["u_right"])
    return a


def _outputs(a, count, key="match_of_cur"):
    """adds the two outputs that every search has to the fields of a frame: a[count] matches and their number"""
    a[key] = np.full(max(a[count], 1), -1, np.int32); a["nmatches"] = np.zeros(1, np.int32)
    return a


def _matches(a, count, key="match_of_cur"):
    return a[key][:a[count]].copy(), int(a["nmatches"][0])


def poseopt_items(items):
    """the sind_poseopt_item array of ORBmatcher.PoseOptimization's items, and the arrays it points to (which live as long as the caller keeps them)"""
    arr = (_PoseOptItem * len(items))(); keep = []
    for q, it in zip(arr, items):
        n = len(it["u_right"])
        a = dict(x3Dw=_f32(it["x3Dw"]), obs_xy=_f32(it["obs_xy"]), u_right=_f32(it["u_right"]), inv_sigma2=_f32(it["inv_sigma2"]), Tcw=_f32(it["Tcw"]).reshape(4, 4).copy())
        a.update(Tcw_out=a["Tcw"].copy(), outlier=np.zeros(n, np.uint8), n_good=np.zeros(1, np.int32), n_rounds=np.zeros(1, np.int32), round_iters=np.zeros(4, np.int32),
                 round_nbad=np.zeros(4, np.int32), round_pose=np.zeros((4, 12), np.float64), round_chi2=np.zeros(4, np.float64), round_lambda=np.zeros(4, np.float64))
        for key, v in a.items():
            setattr(q, key, v.ctypes.data if v.size else None)
        q.n = n
        keep.append(a)
    return arr, keep


def poseopt_result(a):
    return dict(Tcw=a["Tcw_out"], outlier=a["outlier"], n_good=int(a["n_good"][0]), n_rounds=int(a["n_rounds"][0]),
                **{k: a[k] for k in ("round_iters", "round_nbad", "round_pose", "round_chi2", "round_lambda")})


def sim3opt_items(items):
    """the sind_sim3opt_item array of ORBmatcher.OptimizeSim3's items, and the arrays it points to (which live as long as the caller keeps them)"""
    arr = (_Sim3OptItem * len(items))(); keep = []
    for q, it in zip(arr, items):
        n = len(it["inv_sigma2_1"])
        a = dict(x3Dc1=_f32(it["x3Dc1"]), x3Dc2=_f32(it["x3Dc2"]), obs1_xy=_f32(it["obs1_xy"]), obs2_xy=_f32(it["obs2_xy"]), inv_sigma2_1=_f32(it["inv_sigma2_1"]),
                 inv_sigma2_2=_f32(it["inv_sigma2_2"]), K1=_f32(it["K1"]).reshape(4).copy(), K2=_f32(it["K2"]).reshape(4).copy(), R12=_f32(it["R12"]).reshape(3, 3).copy(),
                 t12=_f32(it["t12"]).reshape(3).copy())
        a.update(q_out=np.zeros(4, np.float64), t_out=np.zeros(3, np.float64), s_out=np.zeros(1, np.float64), removed=np.zeros(n, np.uint8), n_inliers=np.zeros(1, np.int32),
                 n_bad=np.zeros(1, np.int32), n_stages=np.zeros(1, np.int32), stage_iters=np.zeros(2, np.int32), stage_chi2=np.zeros(2, np.float64), stage_lambda=np.zeros(2, np.float64))
        for key, v in a.items():
            setattr(q, key, v.ctypes.data if v.size else None)
        q.n = n; q.s12 = float(np.float32(it["s12"]))
        keep.append(a)
    return arr, keep


def sim3opt_result(a):
    return dict(q=a["q_out"], t=a["t_out"], s=np.float64(a["s_out"][0]), removed=a["removed"], n_inliers=int(a["n_inliers"][0]), n_bad=int(a["n_bad"][0]), n_stages=int(a["n_stages"][0]),
                **{k: a[k] for k in ("stage_iters", "stage_chi2", "stage_lambda")})


def localba_items(items):
    """the sind_localba_item array of ORBmatcher.LocalBundleAdjustment's items, and the arrays it points to (which live as long as the caller keeps them)"""
    arr = (_LocalBaItem * len(items))(); keep = []
    for q, it in zip(arr, items):
        n_kf, n_mp = len(it["kf_id"]), len(it["mp_id"])
        a = dict(kf_id=np.ascontiguousarray(it["kf_id"], np.int64), kf_kind=_u8(it["kf_kind"]), Tcw=_f32(it["Tcw"]).reshape(n_kf, 16).copy(), mp_id=np.ascontiguousarray(it["mp_id"], np.int64),
                 x3Dw=_f32(it["x3Dw"]).reshape(n_mp, 3).copy(), obs_start=_i32(it["obs_start"]), obs_kf=_i32(it["obs_kf"]), obs_xy=_f32(it["obs_xy"]), u_right=_f32(it["u_right"]),
                 inv_sigma2=_f32(it["inv_sigma2"]))
        n_obs = len(a["obs_kf"])
        a.update(Tcw_out=a["Tcw"].copy(), x3Dw_out=a["x3Dw"].copy(), erase=np.zeros(n_obs, np.uint8), n_stages=np.zeros(1, np.int32), stage_iters=np.zeros(2, np.int32),
                 n_level1=np.zeros(1, np.int32), stage_chi2=np.zeros(2, np.float64), stage_lambda=np.zeros(2, np.float64))
        for key, v in a.items():
            setattr(q, key, v.ctypes.data if v.size else None)
        q.n_kf = n_kf; q.n_mp = n_mp; q.do_more = int(bool(it.get("do_more", True)))
        keep.append(a)
    return arr, keep


def localba_result(a):
    return dict(Tcw=a["Tcw_out"].reshape(-1, 4, 4), x3Dw=a["x3Dw_out"], erase=a["erase"], n_stages=int(a["n_stages"][0]), n_level1=int(a["n_level1"][0]),
                **{k: a[k] for k in ("stage_iters", "stage_chi2", "stage_lambda")})


def globalba_items(items):
    """the sind_globalba_item array of ORBmatcher.GlobalBundleAdjustment's items, and the arrays it points to (which live as long as the caller keeps them)"""
    arr = (_GlobalBaItem * len(items))(); keep = []
    for q, it in zip(arr, items):
        n_kf, n_mp = len(it["kf_id"]), len(it["mp_id"])
        a = dict(kf_id=np.ascontiguousarray(it["kf_id"], np.int64), Tcw=_f32(it["Tcw"]).reshape(n_kf, 16).copy(), mp_id=np.ascontiguousarray(it["mp_id"], np.int64),
                 x3Dw=_f32(it["x3Dw"]).reshape(n_mp, 3).copy(), obs_start=_i32(it["obs_start"]), obs_kf=_i32(it["obs_kf"]), obs_xy=_f32(it["obs_xy"]), u_right=_f32(it["u_right"]),
                 inv_sigma2=_f32(it["inv_sigma2"]))
        a.update(Tcw_out=a["Tcw"].copy(), x3Dw_out=a["x3Dw"].copy(), included=np.full(n_mp, 255, np.uint8), n_iters=np.zeros(1, np.int32), chi2=np.zeros(1, np.float64),
                 lambda_=np.zeros(1, np.float64), n_active_poses=np.zeros(1, np.int32), solver_fail=np.zeros(1, np.int32), env_entries=np.zeros(1, np.int64),
                 env_dense_entries=np.zeros(1, np.int64))
        for key, v in a.items():
            setattr(q, key, v.ctypes.data if v.size else None)
        q.n_kf = n_kf; q.n_mp = n_mp
        keep.append(a)
    return arr, keep


def globalba_result(a):
    return dict(Tcw=a["Tcw_out"].reshape(-1, 4, 4), x3Dw=a["x3Dw_out"], included=a["included"], n_iters=int(a["n_iters"][0]), chi2=np.float64(a["chi2"][0]), lambda_=np.float64(a["lambda_"][0]),
                n_active_poses=int(a["n_active_poses"][0]), solver_fail=int(a["solver_fail"][0]), env_entries=int(a["env_entries"][0]), env_dense_entries=int(a["env_dense_entries"][0]))


def essgraph_items(items):
    """the sind_essgraph_item array of ORBmatcher.OptimizeEssentialGraph's items, and the arrays it points to (which live as long as the caller keeps them)"""
    arr = (_EssGraphItem * len(items))(); keep = []
    for q, it in zip(arr, items):
        n_kf = len(it["kf_id"])
        a = dict(kf_id=np.ascontiguousarray(it["kf_id"], np.int64), Tcw=_f32(it["Tcw"]).reshape(n_kf, 16).copy(), has_corrected=_u8(it["has_corrected"]),
                 corrected=np.ascontiguousarray(it["corrected"], np.float64).reshape(n_kf, 8), has_noncorrected=_u8(it["has_noncorrected"]),
                 noncorrected=np.ascontiguousarray(it["noncorrected"], np.float64).reshape(n_kf, 8), edge_i=_i32(it["edge_i"]), edge_j=_i32(it["edge_j"]), edge_kind=_u8(it["edge_kind"]),
                 x3Dw=_f32(it["x3Dw"]).reshape(-1, 3).copy(), mp_ref=_i32(it["mp_ref"]))
        a.update(Siw_out=np.zeros((n_kf, 8), np.float64), Tiw_out=a["Tcw"].copy(), x3Dw_out=a["x3Dw"].copy(), n_iters=np.zeros(1, np.int32), chi2=np.zeros(1, np.float64),
                 lambda_=np.zeros(1, np.float64), n_active=np.zeros(1, np.int32), solver_fail=np.zeros(1, np.int32))
        for key, v in a.items():
            setattr(q, key, v.ctypes.data if v.size else None)
        q.n_kf = n_kf; q.n_edges = len(a["edge_i"]); q.n_mp = len(a["mp_ref"]); q.fixed_kf = int(it["fixed_kf"])
        keep.append(a)
    return arr, keep


def essgraph_result(a):
    return dict(Siw=a["Siw_out"], Tiw=a["Tiw_out"].reshape(-1, 4, 4), x3Dw=a["x3Dw_out"], n_iters=int(a["n_iters"][0]), chi2=np.float64(a["chi2"][0]), lambda_=np.float64(a["lambda_"][0]),
                n_active=int(a["n_active"][0]), solver_fail=int(a["solver_fail"][0]))


def triangulate_items(pairs):
    """the sind_tri_pair array of ORBmatcher.Triangulate's pairs, and the arrays it points to (which live as long as the caller keeps them)"""
    arr = (_TriPair * len(pairs))(); keep = []
    for q, it in zip(arr, pairs):
        n1 = len(it["kf1"]["octave"])
        a = dict(Tcw1=_f32(it["Tcw1"]).reshape(4, 4).copy(), Twc1=_f32(it["Twc1"]).reshape(4, 4).copy(), Tcw2=_f32(it["Tcw2"]).reshape(4, 4).copy(), Twc2=_f32(it["Twc2"]).reshape(4, 4).copy(),
                 match12=_i32(it["match12"]), x3D=np.zeros((n1, 3), np.float32), how=np.full(n1, -1, np.int32), status=np.full(n1, -1, np.int32), nnew=np.zeros(1, np.int32))
        for key, v in a.items():
            setattr(q, key, v.ctypes.data if v.size else None)
        for name, side in (("kf1", q.kf1), ("kf2", q.kf2)):
            d = it[name]
            b = dict(xy=_f32(d["xy"]), un_xy=_f32(d["un_xy"]), octave=_i32(d["octave"]), u_right=_f32(d["u_right"]), depth=_f32(d["depth"]))
            side.n = len(b["octave"])
            for key, v in b.items():
                setattr(side, key, v.ctypes.data if v.size else None)
            a[name] = b
        keep.append(a)
    return arr, keep


def triangulate_result(a):
    return dict(x3D=a["x3D"], how=a["how"], status=a["status"], nnew=int(a["nnew"][0]))


def mappoints_items(items):
    """the sind_mappoints_item array of ORBmatcher.UpdateMapPoints's items, and the arrays it points to (which live as long as the caller keeps them).  The outputs start
    from the item's desc, normal, max_dist, min_dist where it has them (what the map holds: the call leaves them where the reference returns early), else from zeros"""
    arr = (_MapPointsItem * len(items))(); keep = []
    for q, it in zip(arr, items):
        n_kf, n_mp = len(it["Ow"]), len(it["x3Dw"])
        a = dict(Ow=_f32(it["Ow"]).reshape(n_kf, 3).copy(), x3Dw=_f32(it["x3Dw"]).reshape(n_mp, 3).copy(), obs_start=_i32(it["obs_start"]), obs_kf=_i32(it["obs_kf"]), obs_bad=_u8(it["obs_bad"]),
                 obs_octave=_i32(it["obs_octave"]), obs_desc=_u8(it["obs_desc"]).reshape(-1, 32), ref_obs=_i32(it["ref_obs"]))
        prior = lambda key, shape, dtype: np.array(it[key], dtype).reshape(shape).copy() if it.get(key) is not None else np.zeros(shape, dtype)
        a.update(desc_out=prior("desc", (n_mp, 32), np.uint8), best_obs=np.full(n_mp, -1, np.int32), normal_out=prior("normal", (n_mp, 3), np.float32),
                 max_dist=prior("max_dist", (n_mp,), np.float32), min_dist=prior("min_dist", (n_mp,), np.float32), updated=np.zeros(n_mp, np.uint8))
        for key, v in a.items():
            setattr(q, key, v.ctypes.data if v.size else None)
        q.n_kf = n_kf; q.n_mp = n_mp; q.do_descriptor = int(bool(it.get("do_descriptor", True))); q.do_normal = int(bool(it.get("do_normal", True)))
        keep.append(a)
    return arr, keep


def mappoints_result(a):
    return dict(desc=a["desc_out"], best_obs=a["best_obs"], normal=a["normal_out"], max_dist=a["max_dist"], min_dist=a["min_dist"], updated=a["updated"])


class ORBmatcher:
    """ORBmatcher(nnratio, checkOri) of the reference.  Provided: SearchByProjection(CurrentFrame, LastFrame, th, bMono) (TrackWithMotionModel),
    SearchLocalPoints = Frame::isInFrustum over the local map + SearchByProjection(F, vpMapPoints, th) (TrackLocalMap), and SearchByProjectionKF =
    SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (Relocalization).  A frame / a set of map points is a dict of arrays
    (see include/sind_hip.h: sind_match_pair, sind_match_local, sind_match_reloc).  By vocabulary node: SearchByBoW(pKF, F) (TrackReferenceKeyFrame, Relocalization;
    :159-288) and SearchForTriangulation (LocalMapping::CreateNewMapPoints; :657-823), on node ids from vocabulary.ORBVocabulary (sind_match_bow, sind_match_tri), and SearchByBoWKF =
    SearchByBoW(pKF1, pKF2) (LoopClosing::ComputeSim3; :522-655; sind_match_bow_kf).  Of ORBmatcher.cc only the monocular SearchForInitialization is not provided.
    On the same handle, between SearchByBoWKF and SearchBySim3 in LoopClosing::ComputeSim3: the Sim3Solver (src/Sim3Solver.cc; Sim3Ransac, sim3_solvers, sindslam_amd/sim3.py).
    Between SearchByBoW and SearchByProjectionKF in Tracking::Relocalization: the PnPsolver (src/PnPsolver.cc; PnPRansac, pnp_solvers, sindslam_amd/pnp.py).
    After every search of the tracking thread: Optimizer::PoseOptimization (src/Optimizer.cc:239-451; PoseOptimization, sindslam_amd/optimizer.py).
    After SearchBySim3 in LoopClosing::ComputeSim3: Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241; OptimizeSim3, sindslam_amd/optimizer.py).
    After SearchInNeighbors in LocalMapping::Run: Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778; LocalBundleAdjustment, sindslam_amd/optimizer.py).
    After the loop fusion in LoopClosing::CorrectLoop: Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044; OptimizeEssentialGraph, sindslam_amd/optimizer.py).
    After CorrectLoop, in LoopClosing::RunGlobalBundleAdjustment: Optimizer::BundleAdjustment (src/Optimizer.cc:49-237; GlobalBundleAdjustment, sindslam_amd/optimizer.py).
    The arithmetic on the map points themselves: after SearchForTriangulation the loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:284-431; Triangulate), and
    MapPoint::ComputeDistinctiveDescriptors with MapPoint::UpdateNormalAndDepth wherever the reference calls the pair (src/MapPoint.cc:242-371; UpdateMapPoints,
    sindslam_amd/mapping.py)."""
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, fx, fy, cx, cy, bf, bounds, scale_factors, nnratio=0.6, checkOri=True, cap=4096, max_batch=1, device=0, cap_points=0):
        cfg = _Config(fx, fy, cx, cy, bf, (C.c_float * 4)(*[float(b) for b in bounds]),
                      (C.c_float * 16)(*([float(s) for s in scale_factors] + [0.0] * (16 - len(scale_factors)))),
                      len(scale_factors), cap, cap, max_batch, device)
        self.checkOri, self.nnratio, self.max_batch = checkOri, nnratio, int(max_batch)
        self.K5 = (float(fx), float(fy), float(cx), float(cy), float(bf))
        h = C.c_void_p()
        check(lib().sind_match_create(C.byref(cfg), C.byref(h)), "sind_match_create")
        self._h = h
        if cap_points:
            self.reserve_map_points(cap_points)

    def close(self):
        if getattr(self, "_h", None):
            lib().sind_match_destroy(self._h); self._h = None

    __del__ = close

    def reserve_map_points(self, cap_points):
        """capacity for local map points per frame; needed once before SearchLocalPoints (or pass cap_points to the constructor)"""
        check(lib().sind_match_reserve_map_points(self._h, int(cap_points)), "sind_match_reserve_map_points")

    def _call(self, name, ctype, items, *args):
        """One call of the C ABI on a batch.  items: per frame, the fields of its struct by name: counts as int, arrays as numpy (an empty one goes as NULL)"""
        arr = (ctype * len(items))()
        for q, a in zip(arr, items):
            for k, v in a.items():
                setattr(q, k, v if isinstance(v, int) else v.ctypes.data if v.size else None)
        check(getattr(lib(), name)(self._h, arr, len(items), *args), name)

    def SearchByProjection(self, pairs, th, bMono=False):
        """pairs: list of (Tcw_cur, Tcw_last, last, cur) -> list of (match_of_cur i32 [n_cur], nmatches)"""
        items = [_outputs(dict(Tcw_cur=_f32(tc), Tcw_last=_f32(tl), n_last=len(last["valid"]), x3Dw=_f32(last["x3Dw"]), last_valid=_u8(last["valid"]), last_has_obs=_u8(last["has_obs"]),
                               last_octave=_i32(last["octave"]), last_angle=_f32(last["angle"]), last_desc=_u8(last["desc"]), **_cur(cur, "angle", "u_right")), "n_cur")
                 for tc, tl, last, cur in pairs]
        self._call("sind_match_by_projection", _Pair, items, C.c_float(th), int(bMono), int(self.checkOri))
        return [_matches(a, "n_cur") for a in items]

    def SearchLocalPoints(self, frames, th, viewingCosLimit=0.5):
        """frames: list of (Tcw, mp, cur); mp: x3Dw, normal, max_dist, min_dist, flags (bit0 candidate, bit1 observed), desc; cur as for SearchByProjection
        (angle unused).  Uses the constructor's nnratio.  -> list of dicts: match_of_cur i32 [n_cur] (index of the map point, -1: none), nmatches,
        in_view u8 [n], proj_xyr f32 [n, 3], level i32 [n], view_cos f32 [n], n_to_match."""
        items = []
        for T, mp, cur in frames:
            n = len(mp["flags"])
            items.append(_outputs(dict(Tcw=_f32(T), n_points=n, x3Dw=_f32(mp["x3Dw"]), normal=_f32(mp["normal"]), max_dist=_f32(mp["max_dist"]), min_dist=_f32(mp["min_dist"]), flags=_u8(mp["flags"]),
                                       desc=_u8(mp["desc"]), in_view=np.zeros(max(n, 1), np.uint8), proj_xyr=np.zeros((max(n, 1), 3), np.float32), level=np.zeros(max(n, 1), np.int32),
                                       view_cos=np.zeros(max(n, 1), np.float32), n_to_match=np.zeros(1, np.int32), **_cur(cur, "u_right")), "n_cur"))
        self._call("sind_match_local_map", _Local, items, C.c_float(th), C.c_float(self.nnratio), C.c_float(viewingCosLimit))
        return [dict(zip(("match_of_cur", "nmatches"), _matches(a, "n_cur")), n_to_match=int(a["n_to_match"][0]),
                     **{k: a[k][:a["n_points"]].copy() for k in ("in_view", "proj_xyr", "level", "view_cos")}) for a in items]

    def SearchByProjectionKF(self, pairs, th, ORBdist):
        """pairs: list of (Tcw_cur, kf, cur); kf, per slot of the key frame: x3Dw, max_dist, min_dist, valid (pMP && !isBad && not already found), angle, desc;
        cur as for SearchByProjection, taken = the keypoint holds any map point.  At most `cap` slots.  -> list of (match_of_cur i32 [n_cur], nmatches)"""
        items = [_outputs(dict(Tcw=_f32(T), n_points=len(kf["valid"]), x3Dw=_f32(kf["x3Dw"]), max_dist=_f32(kf["max_dist"]), min_dist=_f32(kf["min_dist"]), valid=_u8(kf["valid"]),
                               kf_angle=_f32(kf["angle"]), desc=_u8(kf["desc"]), **_cur(cur, "angle")), "n_cur") for T, kf, cur in pairs]
        self._call("sind_match_by_projection_kf", _Reloc, items, C.c_float(th), int(ORBdist), int(self.checkOri))
        return [_matches(a, "n_cur") for a in items]

    def SearchByBoW(self, pairs, nnratio=None):
        """pairs: list of (kf, cur); kf, per keypoint of the key frame: node (as ORBVocabulary.transform returns it), valid (pMP && !isBad), angle, desc (the key
        frame's own descriptors); cur: node, angle, desc.  nnratio None = the constructor's.  -> list of (match_of_cur i32 [n_cur], nmatches)"""
        items = [_outputs(dict(n_kf=len(kf["node"]), kf_node=_i32(kf["node"]), kf_valid=_u8(kf["valid"]), kf_angle=_f32(kf["angle"]), kf_desc=_u8(kf["desc"]),
                               n_cur=len(cur["node"]), cur_node=_i32(cur["node"]), cur_angle=_f32(cur["angle"]), cur_desc=_u8(cur["desc"])), "n_cur") for kf, cur in pairs]
        self._call("sind_match_by_bow", _Bow, items, C.c_float(self.nnratio if nnratio is None else nnratio), int(self.checkOri))
        return [_matches(a, "n_cur") for a in items]

    def SearchByBoWKF(self, pairs, nnratio=None):
        """SearchByBoW(pKF1, pKF2, vpMatches12) (:522-655; LoopClosing::ComputeSim3, one call for all candidates).  pairs: list of (kf1, kf2); either, per keypoint:
        node, valid (pMP && !isBad), angle (mvKeysUn), desc.  nnratio None = the constructor's.  -> list of (match12 i32 [n1] = idx2 or -1, nmatches)"""
        items = []
        for k1, k2 in pairs:
            a = {}
            for s, k in (("1", k1), ("2", k2)):
                a.update({"n" + s: len(k["node"]), "node" + s: _i32(k["node"]), "valid" + s: _u8(k["valid"]), "angle" + s: _f32(k["angle"]), "desc" + s: _u8(k["desc"])})
            items.append(_outputs(a, "n1", "match12"))
        self._call("sind_match_by_bow_kf", _BowKF, items, C.c_float(self.nnratio if nnratio is None else nnratio), int(self.checkOri))
        return [_matches(a, "n1", "match12") for a in items]

    def SearchForTriangulation(self, pairs, bOnlyStereo=False):
        """pairs: list of (Tcw2, Cw1, F12, kf1, kf2); kf1, per keypoint: node, has_mp, un_xy, angle, u_right, desc; kf2: the same and octave.
        -> list of (match12 i32 [n1], nmatches, matched_pairs i64 [nmatches, 2] = vMatchedPairs, ascending idx1)"""
        items = []
        for T2, Cw1, F12, k1, k2 in pairs:
            a = dict(Tcw2=_f32(T2), Cw1=_f32(Cw1), F12=_f32(F12), octave2=_i32(k2["octave"]))
            for s, k in (("1", k1), ("2", k2)):
                a.update({"n" + s: len(k["node"]), "node" + s: _i32(k["node"]), "has_mp" + s: _u8(k["has_mp"]), "un_xy" + s: _f32(k["un_xy"]), "angle" + s: _f32(k["angle"]),
                          "u_right" + s: _f32(k["u_right"]), "desc" + s: _u8(k["desc"])})
            items.append(_outputs(a, "n1", "match12"))
        self._call("sind_match_for_triangulation", _Tri, items, int(bOnlyStereo), int(self.checkOri))
        res = []
        for m, n in (_matches(a, "n1", "match12") for a in items):
            i1 = np.nonzero(m >= 0)[0]
            res.append((m, n, np.stack([i1, m[i1]], 1).astype(np.int64)))
        return res

    def _fuse(self, items, th, sim3):
        its = []
        for T, mp, kf in items:
            a = _points_kf(mp, kf, u_right=not sim3); n = max(a["n_points"], 1)
            a.update(Tcw=_f32(T), best_idx=np.full(n, -1, np.int32), best_dist=np.full(n, -1, np.int32), nfused=np.zeros(1, np.int32))
            its.append(a)
        self._call("sind_match_fuse", _Fuse, its, C.c_float(th), int(sim3))
        return [dict(best_idx=a["best_idx"][:a["n_points"]].copy(), best_dist=a["best_dist"][:a["n_points"]].copy(), nfused=int(a["nfused"][0])) for a in its]

    def Fuse(self, items, th=3.0):
        """Fuse(pKF, vpMapPoints, th) up to its graph tail (:825-949).  items: list of (Tcw, mp, kf); mp, per entry of the list: x3Dw, normal, max_dist, min_dist,
        valid (pMP && !isBad && !IsInKeyFrame(pKF)), desc; kf, per keypoint: un_xy, octave, u_right, desc, grid_start, grid_idx.  Needs cap_points.
        -> list of dicts: best_idx i32 [n] (bestIdx if bestDist <= TH_LOW, else -1), best_dist i32 [n], nfused.  The caller replays the tail."""
        return self._fuse(items, th, 0)

    def FuseSim3(self, items, th):
        """Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) up to its graph tail (:977-1079).  items: list of (Scw, mp, kf) as for Fuse with
        valid = !isBad && !spAlreadyFound.count(pMP); kf["u_right"] is not read.  -> as Fuse"""
        return self._fuse(items, th, 1)

    def SearchByProjectionSim3(self, items, th):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:290-403).  items: list of (Scw, mp, kf) as for FuseSim3; kf["taken"] = vpMatched[idx] != NULL on entry
        (None = none).  th: int.  -> list of (match_of_kf i32 [n_kf] = index of the point written to vpMatched[idx] or -1, nmatches)"""
        its = []
        for S, mp, kf in items:
            a = _points_kf(mp, kf); a["Scw"] = _f32(S)
            if kf.get("taken") is not None:
                a["kf_taken"] = _u8(kf["taken"])
            its.append(_outputs(a, "n_kf", "match_of_kf"))
        self._call("sind_match_by_projection_sim3", _ProjSim3, its, int(th))
        return [_matches(a, "n_kf", "match_of_kf") for a in its]

    def SearchBySim3(self, pairs, th):
        """SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1102-1326).  pairs: list of (T1w, T2w, s12, R12, t12, side1, side2); a side, per slot of the key
        frame: valid (pMP && !isBad && !vbAlreadyMatched), x3Dw, max_dist, min_dist, mp_desc (of the slot's map point), un_xy, octave, kf_desc (of the slot's keypoint),
        and grid_start, grid_idx.  -> list of (match12 i32 [n1] = idx2 where both directions agree or -1, nfound)"""
        arr = (_Sim3Pair * len(pairs))(); keep = []
        for q, (T1, T2, s12, R12, t12, s1, s2) in zip(arr, pairs):
            a = dict(T1w=_f32(T1), T2w=_f32(T2), R12=_f32(R12), t12=_f32(t12), match12=np.full(max(len(s1["valid"]), 1), -1, np.int32), nfound=np.zeros(1, np.int32))
            for k, v in a.items():
                setattr(q, k, v.ctypes.data)
            q.s12 = float(s12)
            for name, side, d in (("side1", q.side1, s1), ("side2", q.side2, s2)):
                b = dict(valid=_u8(d["valid"]), x3Dw=_f32(d["x3Dw"]), max_dist=_f32(d["max_dist"]), min_dist=_f32(d["min_dist"]), mp_desc=_u8(d["mp_desc"]), un_xy=_f32(d["un_xy"]),
                         octave=_i32(d["octave"]), kf_desc=_u8(d["kf_desc"]), grid_start=_i32(d["grid_start"]), grid_idx=_i32(d["grid_idx"]))
                side.n = len(d["valid"])
                for k, v in b.items():
                    setattr(side, k, v.ctypes.data if v.size else None)
                a[name] = b                                           # the arrays live as long as the call
            a["n1"] = len(s1["valid"]); keep.append(a)
        check(lib().sind_match_by_sim3(self._h, arr, len(pairs), C.c_float(th)), "sind_match_by_sim3")
        return [(a["match12"][:a["n1"]].copy(), int(a["nfound"][0])) for a in keep]

    def Sim3Ransac(self, items, bFixScale):
        """sind_match_sim3_ransac: ComputeSim3 + CheckInliers (src/Sim3Solver.cc:226-364) of every given sample of every candidate, one call.  items: list of (inp, triples);
        inp: T1w, T2w and, per correspondence, x3Dw1, x3Dw2, sigma2_1, sigma2_2; triples i32 [k, 3] into the correspondences.
        -> list of dicts: count i32 [k], bits u64 [k, ceil(n / 64)], s12 f32 [k], R12 f32 [k, 3, 3], t12 f32 [k, 3]"""
        its = []
        for inp, tri in items:
            n, k = len(inp["sigma2_1"]), len(tri)
            its.append(dict(T1w=_f32(inp["T1w"]), T2w=_f32(inp["T2w"]), n=n, x3Dw1=_f32(inp["x3Dw1"]), x3Dw2=_f32(inp["x3Dw2"]), sigma2_1=_f32(inp["sigma2_1"]), sigma2_2=_f32(inp["sigma2_2"]),
                            n_its=k, triple=_i32(tri), count=np.zeros(k, np.int32), inlier_bits=np.zeros((k, (n + 63) // 64), np.uint64), s12=np.zeros(k, np.float32),
                            R12=np.zeros((k, 3, 3), np.float32), t12=np.zeros((k, 3), np.float32)))
        self._call("sind_match_sim3_ransac", _Sim3Item, its, int(bool(bFixScale)))
        return [dict(count=a["count"], bits=a["inlier_bits"], s12=a["s12"], R12=a["R12"], t12=a["t12"]) for a in its]

    def sim3_solvers(self, candidates, bFixScale, rand, rand_max=2147483647):
        """The Sim3Solvers of LoopClosing::ComputeSim3 (src/LoopClosing.cc:252-280), on one tape of `rand`'s raw values and on this handle.  candidates: per initial candidate
        None (vbDiscarded: a bad key frame, fewer than 20 matches) or the flattened constructor (src/Sim3Solver.cc:37-112): T1w, T2w, and per correspondence that passes :64-79, in i1
        order: x3Dw1, x3Dw2, sigma2_1, sigma2_2, indices1 (= i1, mvnIndices1); N1 = vpMatched12.size().  -> list of sim3.Sim3Solver or None, for sim3.compute_sim3"""
        from .sim3 import Sim3Solver, Tape
        tape = Tape(rand, rand_max)
        evaluate = lambda requests, fix: self.Sim3Ransac([(s.inp, tri) for s, tri in requests], fix)
        return [None if c is None else Sim3Solver(evaluate, tape, c, bFixScale) for c in candidates]

    def PnPRansac(self, items):
        """sind_match_pnp_ransac: EPnP + CheckInliers (src/PnPsolver.cc:308-339, :375-950) of every given sample of every candidate and of the Refine problems (:260-305)
        that follow from the counts, one call, all on the device.  items: list of (inp, samples, min_inliers, best_count, best_bits); inp, per correspondence: x3Dw, p2d,
        sigma2, and th2; samples i32 [k, 4] into the correspondences; min_inliers = mRansacMinInliers; best_count, best_bits (u64 words or None) = mnBestInliers,
        mvbBestInliers held from earlier calls.  -> list of dicts: count i32 [k], bits u64 [k, ceil(n / 64)], R f64 [k, 3, 3], t f64 [k, 3], refine i32 [k] (row of the
        refine_* arrays or -1), refine_hyp i32 [r], refine_count i32 [r], refine_bits u64 [r, words], refine_R f64 [r, 3, 3], refine_t f64 [r, 3]"""
        arr = (_PnpItem * len(items))(); keep = []
        for q, (inp, samples, min_inliers, best_count, best_bits) in zip(arr, items):
            n, k = len(inp["sigma2"]), len(samples); w = (n + 63) // 64
            a = dict(x3Dw=_f32(inp["x3Dw"]), p2d=_f32(inp["p2d"]), sigma2=_f32(inp["sigma2"]), samples=_i32(samples), count=np.zeros(k, np.int32), inlier_bits=np.zeros((k, w), np.uint64),
                     R=np.zeros((k, 3, 3), np.float64), t=np.zeros((k, 3), np.float64), refine=np.full(k, -1, np.int32), n_refines=np.zeros(1, np.int32), refine_hyp=np.full(k + 1, -1, np.int32),
                     refine_count=np.zeros(k + 1, np.int32), refine_bits=np.zeros((k + 1, w), np.uint64), refine_R=np.zeros((k + 1, 3, 3), np.float64), refine_t=np.zeros((k + 1, 3), np.float64))
            if best_bits is not None:
                a["best_bits"] = np.ascontiguousarray(best_bits, np.uint64)
            for key, v in a.items():
                setattr(q, key, v.ctypes.data if v.size else None)
            q.n, q.n_its, q.th2, q.min_inliers, q.best_count = n, k, float(inp["th2"]), int(min_inliers), int(best_count)
            keep.append(a)
        check(lib().sind_match_pnp_ransac(self._h, arr, len(items)), "sind_match_pnp_ransac")
        out = []
        for a in keep:
            r = int(a["n_refines"][0])
            out.append(dict(count=a["count"], bits=a["inlier_bits"], R=a["R"], t=a["t"], refine=a["refine"], **{key: a[key][:r] for key in ("refine_hyp", "refine_count", "refine_bits", "refine_R", "refine_t")}))
        return out

    def pnp_solvers(self, candidates, rand, rand_max=2147483647):
        """The PnPsolvers of Tracking::Relocalization (src/Tracking.cc:1407-1428), on one tape of `rand`'s raw values and on this handle.  candidates: per candidate None
        (vbDiscarded: a bad key frame, fewer than 15 matches) or the flattened constructor (src/PnPsolver.cc:67-110): per keypoint i with pMP && !pMP->isBad(), in ascending i:
        x3Dw, p2d, sigma2, indices (= i, mvKeyPointIndices); n_keypoints = vpMapPointMatches.size().  -> list of pnp.PnPsolver or None, for pnp.relocalization_pnp.
        Every solver has the header's default parameters; Relocalization calls SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) on each."""
        from .pnp import PnPsolver
        from .sim3 import Tape
        tape = Tape(rand, rand_max)
        solvers = [None if c is None else PnPsolver(self.PnPRansac, tape, c) for c in candidates]
        for s in solvers:
            if s is not None:
                s.max_batch = self.max_batch                            # relocalization_pnp evaluates that many candidates per call
        return solvers

    def PoseOptimization(self, items):
        """sind_match_pose_optimize: Optimizer::PoseOptimization (src/Optimizer.cc:239-451) of every item, one launch.  items: list of dicts, per correspondence (keypoint i
        with mvpMapPoints[i] != NULL, ascending i): x3Dw [n, 3], obs_xy [n, 2], u_right [n] (< 0: monocular edge), inv_sigma2 [n]; and Tcw [4, 4] = mTcw on entry.
        -> list of dicts: Tcw f32 [4, 4] (the pose SetPose gets; the input pose where n < 3, which the reference leaves untouched), outlier u8 [n], n_good, n_rounds,
        round_iters i32 [4], round_nbad i32 [4], round_pose f64 [4, 12], round_chi2 f64 [4], round_lambda f64 [4]"""
        arr, keep = poseopt_items(items)
        check(lib().sind_match_pose_optimize(self._h, arr, len(items)), "sind_match_pose_optimize")
        return [poseopt_result(a) for a in keep]

    def OptimizeSim3(self, items, th2=10, fix_scale=True):
        """sind_match_sim3_optimize: Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) of every item, one launch.  items: list of dicts, per correspondence (the pairs that
        pass :1099-1136, ascending i): x3Dc1, x3Dc2 [n, 3] (the map points in their own cameras), obs1_xy, obs2_xy [n, 2], inv_sigma2_1, inv_sigma2_2 [n]; and K1, K2 [4]
        (fx fy cx cy), s12, R12 [3, 3], t12 [3] = g2oS12 on entry.  th2 and fix_scale as in the reference (10 and mbFixScale in LoopClosing).
        -> list of dicts: q f64 [4] (x y z w, not normalised), t f64 [3], s f64 = g2oS12 afterwards (the input where 0 is returned early), removed u8 [n] (1 where
        vpMatches1[idx] was nulled), n_inliers (the return value), n_bad, n_stages, stage_iters i32 [2], stage_chi2 f64 [2], stage_lambda f64 [2]"""
        arr, keep = sim3opt_items(items)
        check(lib().sind_match_sim3_optimize(self._h, arr, len(items), C.c_float(float(th2)), int(bool(fix_scale))), "sind_match_sim3_optimize")
        return [sim3opt_result(a) for a in keep]

    def LocalBundleAdjustment(self, items):
        """sind_match_local_ba: Optimizer::LocalBundleAdjustment (src/Optimizer.cc:506-743) of every item, one launch.  items: list of dicts: kf_id i64 [n_kf], kf_kind u8 [n_kf]
        (0 local, 1 local and fixed, 2 fixed camera), Tcw [n_kf, 4, 4]; mp_id i64 [n_mp], x3Dw [n_mp, 3]; obs_start i32 [n_mp + 1], and per observation in the order the edges
        are added obs_kf i32 (index into the key frames), obs_xy [n_obs, 2], u_right [n_obs] (< 0: monocular edge), inv_sigma2 [n_obs]; do_more (default True).
        -> list of dicts: Tcw f32 [n_kf, 4, 4] (what SetPose gets; a fixed camera's row is its input), x3Dw f32 [n_mp, 3], erase u8 [n_obs] (vToErase), n_stages, n_level1,
        stage_iters i32 [2], stage_chi2 f64 [2], stage_lambda f64 [2].  The lists the kernel walks are built inside the call."""
        arr, keep = localba_items(items)
        check(lib().sind_match_local_ba(self._h, arr, len(items)), "sind_match_local_ba")
        return [localba_result(a) for a in keep]

    def OptimizeEssentialGraph(self, items, fix_scale=True):
        """sind_match_essential_graph: Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:787-1043) of every item: the pose graph in one launch, the points in a second one on
        the same stream.  items: list of dicts: kf_id i64 [n_kf] strictly ascending, Tcw [n_kf, 4, 4], has_corrected u8 [n_kf], corrected f64 [n_kf, 8] (qx qy qz qw tx ty tz s),
        has_noncorrected, noncorrected alike, fixed_kf (index of pLoopKF); edge_i, edge_j i32 [n_edges] (vertex 0, vertex 1), edge_kind u8 (0 LoopConnections, 1 normal) in the
        order the edges are added; x3Dw [n_mp, 3], mp_ref i32 [n_mp] (index of the key frame of nIDr).  fix_scale as in the reference (mbFixScale: true for RGB-D).
        -> list of dicts: Siw f64 [n_kf, 8], Tiw f32 [n_kf, 4, 4] (what SetPose gets), x3Dw f32 [n_mp, 3] (what SetWorldPos gets), n_iters, chi2, lambda_, n_active, solver_fail."""
        arr, keep = essgraph_items(items)
        check(lib().sind_match_essential_graph(self._h, arr, len(items), int(bool(fix_scale))), "sind_match_essential_graph")
        return [essgraph_result(a) for a in keep]

    def GlobalBundleAdjustment(self, items, iterations=10, robust=False):
        """sind_match_global_ba: Optimizer::BundleAdjustment (src/Optimizer.cc:49-191, what GlobalBundleAdjustemnt forwards to) of every item, one after the other, each as
        kernels per phase over the whole grid.  items: list of dicts: kf_id i64 [n_kf] strictly ascending (the key frame with id 0 is fixed), Tcw [n_kf, 4, 4]; mp_id i64 [n_mp],
        x3Dw [n_mp, 3]; obs_start i32 [n_mp + 1], and per observation in the order the edges are added obs_kf i32 (index into the key frames), obs_xy [n_obs, 2], u_right [n_obs]
        (< 0: monocular edge), inv_sigma2 [n_obs].  iterations: 10 in loop closing, 20 the reference's default, 0 = the stop flag set at entry.  robust: bRobust.
        -> list of dicts: Tcw f32 [n_kf, 4, 4], x3Dw f32 [n_mp, 3], included u8 [n_mp] (0: a point without observations, vbNotIncludedMP), n_iters, chi2, lambda_,
        n_active_poses, solver_fail, env_entries, env_dense_entries."""
        arr, keep = globalba_items(items)
        check(lib().sind_match_global_ba(self._h, arr, len(items), int(iterations), int(bool(robust))), "sind_match_global_ba")
        return [globalba_result(a) for a in keep]

    def Triangulate(self, pairs):
        """sind_match_triangulate: the per-match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:284-431) for every pair, one launch.  pairs: list of dicts: Tcw1,
        Twc1 (GetPose(), GetPoseInverse() of the current key frame), Tcw2, Twc2 (the neighbour's), kf1 and kf2 = dicts per keypoint of xy (mvKeys), un_xy (mvKeysUn), octave,
        u_right, depth, and match12 i32 [n1] as SearchForTriangulation returns it.  -> list of dicts: x3D f32 [n1, 3], how i32 [n1] (0 triangulated, 1 / 2 UnprojectStereo of
        key frame 1 / 2, -1 none), status i32 [n1] (0 a new point, 1..8 the `continue` that rejected the match in source order, -1 no match), nnew"""
        arr, keep = triangulate_items(pairs)
        check(lib().sind_match_triangulate(self._h, arr, len(pairs)), "sind_match_triangulate")
        return [triangulate_result(a) for a in keep]

    def UpdateMapPoints(self, items):
        """sind_match_update_points: MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:242-307, :330-371) of every point of every item,
        two launches and one wait.  items: list of dicts: Ow [n_kf, 3] (GetCameraCenter()), x3Dw [n_mp, 3], obs_start i32 [n_mp + 1], and per observation in the order the
        map iterates obs_kf i32 (index into Ow), obs_bad u8 (pKF->isBad()), obs_octave i32, obs_desc u8 [n_obs, 32]; ref_obs i32 [n_mp] (the position of mpRefKF in the point's
        own list); do_descriptor, do_normal (default True); optionally desc, normal, max_dist, min_dist = what the map holds.
        -> list of dicts: desc u8 [n_mp, 32], best_obs i32 [n_mp] (-1: mDescriptor stays), normal f32 [n_mp, 3], max_dist, min_dist f32 [n_mp], updated u8 [n_mp]"""
        arr, keep = mappoints_items(items)
        check(lib().sind_match_update_points(self._h, arr, len(items)), "sind_match_update_points")
        return [mappoints_result(a) for a in keep]

    def global_ba_counts(self):
        """-> (kernel launches, host waits) of the last GlobalBundleAdjustment on this handle"""
        a, b = C.c_longlong(), C.c_longlong()
        check(lib().sind_match_global_ba_counts(self._h, C.byref(a), C.byref(b)), "sind_match_global_ba_counts")
        return a.value, b.value

    def last_rounds(self):
        return lib().sind_match_last_rounds(self._h)
