"""Scenes for the OptimizeSim3 tests: two cameras with a known Sim3 between them (X1c = s R X2c + t), points in front of both, their observations in both images with
pixel noise and planted gross outliers (in image 1 only, in image 2 only, in both), an input Sim3 near the truth; the degenerate scenes; and the host library's
sindh_sim3_optimize behind the interface of ORBmatcher.OptimizeSim3.  An item is the flattened pair of key frames of include/sind_hip.h, sind_sim3opt_item."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import pnp_scene as S
from poseopt_scene import INV_SIGMA2, bits  # noqa: F401  (bits is used by the tests through this module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1 = np.array(S.K, np.float32)
K2 = np.array((517.3, 516.5, 318.6, 255.3), np.float32)                 # another camera (TUM1), so that cam_map1 and cam_map2 cannot be swapped unnoticed
OUTPUTS = ("q", "t", "s", "removed", "n_inliers", "n_bad", "n_stages", "stage_iters", "stage_chi2", "stage_lambda")
_host = None


def project(K, X):
    return np.stack([K[2] + K[0] * X[:, 0] / X[:, 2], K[3] + K[1] * X[:, 1] / X[:, 2]], 1)


def scene(seed, n, outliers=0.3, noise=0.5, scale=1.0, start=(0.03, 0.03, 0.0)):
    """-> item dict (x3Dc1, x3Dc2, obs1_xy, obs2_xy, inv_sigma2_1, inv_sigma2_2, K1, K2, s12, R12, t12) with the truth beside it (R, t, s, is_outlier, outlier_side).
    outliers: a share (float) or a number (int); outlier k is gross in image 1 (k % 3 == 0), in image 2 (1) or in both (2): the observation is drawn anew, at least 30 px
    from where the point projects.  start: the input Sim3 is the truth turned by that angle, shifted by that much and scaled by 1 + that much"""
    rng = np.random.default_rng(seed)
    R, t = S.pose(rng, 0.3, 0.4)
    X2 = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3, 7, n)], 1).astype(np.float32)
    X1 = (scale * (X2.astype(np.float64) @ R.T) + t).astype(np.float32)
    k1, k2 = K1.astype(np.float64), K2.astype(np.float64)
    uv1 = project(k1, scale * (X2.astype(np.float64) @ R.T) + t)       # where S12 maps the (rounded) point of camera 2: what the noise-free optimum reproduces up to
    uv2 = project(k2, ((X1.astype(np.float64) - t) @ R) / scale)       # the FP32 rounding of the other point
    out = np.zeros(n, bool)
    if isinstance(outliers, int):
        out[rng.choice(n, outliers, replace=False)] = True
    else:
        out = rng.random(n) < outliers
    side = np.full(n, -1)
    obs1 = uv1 + (rng.normal(0, noise, (n, 2)) if noise > 0 else 0.0); obs2 = uv2 + (rng.normal(0, noise, (n, 2)) if noise > 0 else 0.0)
    for k, i in enumerate(np.nonzero(out)[0]):
        side[i] = k % 3
        for obs, uv, hit in ((obs1, uv1, side[i] != 1), (obs2, uv2, side[i] != 0)):
            while hit and np.abs(obs[i] - uv[i]).max() < 30:
                obs[i] = (rng.uniform(0, 640), rng.uniform(0, 480))
    dR, dt = S.pose(np.random.default_rng(seed + 1000), start[0], start[1])
    return dict(x3Dc1=X1, x3Dc2=X2, obs1_xy=obs1.astype(np.float32), obs2_xy=obs2.astype(np.float32), inv_sigma2_1=INV_SIGMA2[rng.integers(0, 4, n)],
                inv_sigma2_2=INV_SIGMA2[rng.integers(0, 4, n)], K1=K1, K2=K2, s12=np.float32(scale * (1 + start[2])), R12=(dR @ R).astype(np.float32), t12=(dR @ t + dt).astype(np.float32),
                R=R, t=t, s=scale, is_outlier=out, outlier_side=side)


def depth_zero(seed=40, n=12):
    """one point of camera 2 that the input Sim3 (identity) maps to depth 0 in camera 1: its error is infinite or NaN from the first linearisation on"""
    s = scene(seed, n, outliers=0, noise=0.3)
    s["x3Dc2"] = s["x3Dc1"].copy(); s["R12"] = np.eye(3, dtype=np.float32); s["t12"] = np.zeros(3, np.float32); s["s12"] = np.float32(1)
    s["x3Dc2"][4] = (0.25, -0.5, 0.0)
    return s


def identical_points(n=12):
    """n times the same pair: every Jacobian is the same, H is rank-deficient"""
    s = scene(41, n, outliers=0, noise=0.0)
    for k in ("x3Dc1", "x3Dc2", "obs1_xy", "obs2_xy", "inv_sigma2_1", "inv_sigma2_2"):
        s[k][:] = s[k][0]
    return s


def exact_identity(n=12):
    """the identity as input and data it explains exactly (the same points in both cameras, observations that are exact in FP32): every error is 0, so is rho"""
    rng = np.random.default_rng(42)
    X = np.stack([rng.integers(-2, 3, n), rng.integers(-2, 3, n), np.full(n, 4)], 1).astype(np.float32)
    K = np.array((512, 512, 320, 240), np.float32)
    uv = project(K.astype(np.float64), X.astype(np.float64)).astype(np.float32)
    one = np.ones(n, np.float32)
    return dict(x3Dc1=X, x3Dc2=X.copy(), obs1_xy=uv, obs2_xy=uv.copy(), inv_sigma2_1=one, inv_sigma2_2=one.copy(), K1=K, K2=K.copy(), s12=np.float32(1), R12=np.eye(3, dtype=np.float32),
                t12=np.zeros(3, np.float32))


def degenerates():
    return dict(depth_zero=depth_zero(), identical_points=identical_points(), exact_identity=exact_identity())


def host():
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(ROOT, "sindslam_amd", "libsind_host.so"))
        _host.sindh_sim3_optimize.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int]
    return _host


class HostOptimizer:
    """sindh_sim3_optimize with the interface of ORBmatcher.OptimizeSim3 (items -> list of result dicts)"""

    def OptimizeSim3(self, items, th2=10, fix_scale=True):
        from sindslam_amd.matcher import sim3opt_items, sim3opt_result
        arr, keep = sim3opt_items(items)
        rc = host().sindh_sim3_optimize(arr, len(items), float(th2), int(bool(fix_scale)))
        assert rc == 0, rc
        return [sim3opt_result(a) for a in keep]


def assert_same(got, ref, what):
    """every output of the call, as bit patterns"""
    for k in OUTPUTS:
        g = np.asarray(got[k]); r = np.asarray(ref[k])
        r = r.astype(g.dtype) if r.dtype.kind in "iub" else r
        assert g.shape == r.reshape(g.shape).shape and np.array_equal(bits(g), bits(r.reshape(g.shape))), (what, k, got[k], ref[k])


def rotation(q):
    """the rotation matrix of a quaternion x y z w, normalised first"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def distance(r, truth):
    """the largest difference over the entries of [s R | t] between a result and the scene's truth"""
    return max(np.abs(float(r["s"]) * rotation(r["q"]) - truth["s"] * truth["R"]).max(), np.abs(np.asarray(r["t"]) - truth["t"]).max())


# ---------------------------------------------------------------- key frames of the synthetic stream for LoopClosing::ComputeSim3
def stream_key_frame(stream, t, slot, drift=1.0, rigid=None, few=None, noise=0.0, obs_noise=0.0, seed=0):
    """Frame t of the stream as a key frame dict of sindslam_amd/optimizer.py: every keypoint with a depth holds a map point, its depth back-projected with the
    ground-truth pose, in a map that has drifted: a point P of the true world is drift * (Rd P + td) there, rigid = (Rd, td), and the pose goes with it.  few: only that many
    slots hold a map point; noise: the map points are off by that much (a standard deviation, in units of the map); obs_noise: the keypoints are that many pixels off the
    places their map points were made from (the map stays consistent in 3-D, which is all the Sim3Solver looks at; OptimizeSim3 compares with the keypoints).  Map-point
    ids are 10000 * slot + keypoint."""
    import bow_scene as B
    import match_scene as M
    import sim3_scene as S3
    f = B.stream_frame(stream, t); cam = f["cam"]
    keys = M.stream_pair(stream, t, seed=t)[5]
    assert np.array_equal(keys["un_xy"], f["un_xy"])
    rng = np.random.default_rng(8000 + seed + t)
    n = len(f["octave"])
    z = f["depth"].astype(np.float64); xy = f["un_xy"].astype(np.float64); T = f["Tcw"].astype(np.float64)
    has = z > 0
    if few is not None:
        has = np.zeros(n, bool); has[rng.permutation(np.nonzero(z > 0)[0])[:few]] = True
    Xc = np.stack([(xy[:, 0] - cam[2]) * z / cam[0], (xy[:, 1] - cam[3]) * z / cam[1], z], 1)
    Rd, td = (np.eye(3), np.zeros(3)) if rigid is None else (np.asarray(rigid[0], np.float64), np.asarray(rigid[1], np.float64))
    to_map = lambda P: drift * (P @ Rd.T + td)
    Xw = to_map((Xc - T[:3, 3]) @ T[:3, :3]) + (rng.normal(0, noise, (n, 3)) if noise > 0 else 0.0)
    Td = np.eye(4); Td[:3, :3] = T[:3, :3] @ Rd.T; Td[:3, 3] = drift * (T[:3, 3] - Td[:3, :3] @ td)
    kf = dict(un_xy=f["un_xy"], octave=f["octave"], angle=f["angle"], inv_sigma2=(np.float32(1.0) / S3.sigma2_of(f["octave"]).astype(np.float32)).astype(np.float32), bad=np.zeros(n, np.uint8),
              Tcw=Td.astype(np.float32), K=np.array(cam[:4], np.float32), mp_desc=f["desc"], kf_desc=f["desc"], desc=f["desc"], grid_start=keys["grid_start"], grid_idx=keys["grid_idx"],
              node=B.stream_nodes(stream, t), slot=slot, true_Tcw=T, drift=drift, rigid=(Rd, td), to_map=to_map, true_Xw=(Xc - T[:3, 3]) @ T[:3, :3])
    if obs_noise > 0:
        import oracle_lib as O
        xy = np.clip(f["un_xy"].astype(np.float64) + rng.normal(0, obs_noise, (n, 2)), (2, 2), (637, 477)).astype(np.float32)
        cal = [stream.fx, stream.fy, stream.cx, stream.cy, 0, 0, 0, 0, 0, 40.0, 1.0 / stream.depth_factor]
        post = O.frame_post_orb(cal, xy[:, 0].copy(), xy[:, 1].copy(), stream.frames(t, 1)[1][0])
        kf.update(un_xy=post["keys_un"], grid_start=post["grid_start"], grid_idx=post["grid_idx"])
    return set_map(kf, has, Xw)


def set_map(kf, has, Xw):
    """the key frame with these map points (world coordinates of its own map) in the slots `has`"""
    import localmap_scene as L
    import match_scene as M
    T = kf["Tcw"].astype(np.float64); n = len(has)
    Xw = np.where(has[:, None], Xw, (0.0, 0.0, 1.0))
    PO = Xw - (-T[:3, :3].T @ T[:3, 3]); d = np.linalg.norm(PO, axis=1)
    mx, mn = L._invariance(d, kf["octave"], M._scale_factors())
    kf = dict(kf, x3Dw=Xw.astype(np.float32), normal=(PO / np.maximum(d, 1e-12)[:, None]).astype(np.float32), max_dist=mx, min_dist=mn, valid=has.astype(np.uint8),
              mp=np.where(has, 10000 * kf["slot"] + np.arange(n), -1).astype(np.int64))
    return kf


def ideal_pair(kf1, kf2, right=3.0, apart=12.0):
    """The two key frames on a map that is exact for each other: a keypoint of pKF1 and one of pKF2 that show the same point (either's back-projection lands within
    `right` px of the other, mutually nearest), no other chosen pair within `apart` px in either image.  pKF1's map point is then pKF2's back-projection and the other
    way round, so with the true Sim3 both edges of the pair have error 0 up to the FP32 rounding of the points; the other slots hold no map point, and a wrong match
    between chosen slots is off by more than `apart` px.  -> kf1, kf2, pairs [k, 2]"""
    def project(kf, Pw):
        T = kf["true_Tcw"]; K = kf["K"].astype(np.float64)
        Xc = Pw @ T[:3, :3].T + T[:3, 3]
        return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1)
    P1, P2 = kf1["true_Xw"], kf2["true_Xw"]
    h1, h2 = kf1["valid"].astype(bool), kf2["valid"].astype(bool)
    uv12 = project(kf2, P1); uv21 = project(kf1, P2)
    xy1, xy2 = kf1["un_xy"].astype(np.float64), kf2["un_xy"].astype(np.float64)
    d12 = np.linalg.norm(uv12[:, None, :] - xy2[None, :, :], axis=2); d12[:, ~h2] = np.inf; d12[~h1] = np.inf      # [n1, n2]: point of slot i1 seen in image 2 against keypoint i2
    d21 = np.linalg.norm(uv21[None, :, :] - xy1[:, None, :], axis=2); d21[:, ~h2] = np.inf; d21[~h1] = np.inf
    pairs = []
    for i1 in np.argsort(d12.min(axis=1)):
        i2 = int(np.argmin(d12[i1]))
        if not (d12[i1, i2] <= right and d21[i1, i2] <= right and int(np.argmin(d12[:, i2])) == i1):
            continue
        if all(np.linalg.norm(xy1[i1] - xy1[a]) > apart and np.linalg.norm(xy2[i2] - xy2[b]) > apart for a, b in pairs):
            pairs.append((int(i1), i2))
    pairs = np.array(pairs, np.int64)
    has1 = np.zeros(len(h1), bool); has1[pairs[:, 0]] = True; has2 = np.zeros(len(h2), bool); has2[pairs[:, 1]] = True
    X1 = np.zeros((len(h1), 3)); X1[pairs[:, 0]] = kf1["to_map"](P2[pairs[:, 1]])
    X2 = np.zeros((len(h2), 3)); X2[pairs[:, 1]] = kf2["to_map"](P1[pairs[:, 0]])
    return set_map(kf1, has1, X1), set_map(kf2, has2, X2), pairs


def true_scw(kf1, kf2):
    """mScw of pKF1 (whose own map is the true world) in pKF2's map: a point P' = drift (Rd P + td) of that map is R1 P + t1 in pKF1's camera"""
    Rd, td = kf2["rigid"]; T1 = kf1["true_Tcw"]
    T = np.eye(4); T[:3, :3] = T1[:3, :3] @ Rd.T / kf2["drift"]; T[:3, 3] = T1[:3, 3] - T1[:3, :3] @ Rd.T @ td
    return T


def sim3_solver_input(kf1, kf2, match12):
    """the flattened Sim3Solver constructor (src/Sim3Solver.cc:37-112) from two key-frame dicts and SearchByBoW's matches"""
    import sim3_scene as S3
    i1 = np.nonzero(match12[:len(kf1["mp"])] >= 0)[0]; i2 = match12[i1]
    return dict(T1w=kf1["Tcw"], T2w=kf2["Tcw"], x3Dw1=kf1["x3Dw"][i1], x3Dw2=kf2["x3Dw"][i2], sigma2_1=S3.sigma2_of(kf1["octave"][i1]), sigma2_2=S3.sigma2_of(kf2["octave"][i2]), indices1=i1,
                N1=len(kf1["mp"]), K=tuple(np.float32(c) for c in kf1["K"]))
