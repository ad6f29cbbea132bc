"""Scenes for the PoseOptimization tests: map points in front of a ground-truth camera, their observations (mono: u_right = -1, stereo: u_right = u - bf / z) with
pixel noise and planted gross outliers, an input pose near the truth; the degenerate scenes; and the host library's sindh_pose_optimize behind the interface of
ORBmatcher.PoseOptimization.  An item is the flattened frame of include/sind_hip.h, sind_poseopt_item."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import pnp_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = 40.0
K5 = tuple(S.K) + (BF,)                                                # fx fy cx cy bf
INV_SIGMA2 = (np.float32(1.0) / S.SIGMA2).astype(np.float32)           # mvInvLevelSigma2
OUTPUTS = ("Tcw", "outlier", "n_good", "n_rounds", "round_iters", "round_nbad", "round_pose", "round_chi2", "round_lambda")
_host = None


def tcw(R, t):
    T = np.eye(4, dtype=np.float32); T[:3, :3] = R; T[:3, 3] = t
    return T


def scene(seed, n, kind="mixed", outliers=0.3, noise=0.5, start=(0.02, 0.03)):
    """-> item dict (x3Dw, obs_xy, u_right, inv_sigma2, Tcw) with the truth beside it (R, t, is_outlier).  kind: mono, stereo or mixed.  outliers: a share (float) or a number
    (int); an outlier's observation is drawn anew, at least 30 px from where the point projects.  start: the input pose is the truth turned by that angle and shifted by that much"""
    rng = np.random.default_rng(seed)
    R, t = S.pose(rng)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 8, n)], 1)
    Xw = ((Xc - t) @ R).astype(np.float32)
    Xc = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([K5[2] + K5[0] * Xc[:, 0] / Xc[:, 2], K5[3] + K5[1] * Xc[:, 1] / Xc[:, 2]], 1)
    out = np.zeros(n, bool)
    if isinstance(outliers, int):
        out[rng.choice(n, outliers, replace=False)] = True
    else:
        out = rng.random(n) < outliers
    obs = uv + (rng.normal(0, noise, (n, 2)) if noise > 0 else 0.0)
    for i in np.nonzero(out)[0]:
        while np.abs(obs[i] - uv[i]).max() < 30:
            obs[i] = (rng.uniform(0, 640), rng.uniform(0, 480))
    stereo = {"mono": np.zeros(n, bool), "stereo": np.ones(n, bool), "mixed": rng.random(n) < 0.5}[kind]
    ur = np.where(stereo, obs[:, 0] - BF / Xc[:, 2] + (rng.normal(0, noise, n) if noise > 0 else 0.0), -1.0)
    dR, dt = S.pose(np.random.default_rng(seed + 1000), *start)
    return dict(x3Dw=Xw, obs_xy=obs.astype(np.float32), u_right=ur.astype(np.float32), inv_sigma2=INV_SIGMA2[rng.integers(0, 8, n)], Tcw=tcw(dR @ R, dR @ t + dt),
                R=R, t=t, is_outlier=out)


def behind_camera(seed=40, n=12):
    """one point exactly at depth 0 under the input pose (identity): its chi2 is infinite or NaN from the first linearisation on"""
    s = scene(seed, n, "mixed", outliers=0, noise=0.3)
    X = s["x3Dw"].astype(np.float64) @ s["R"].T + s["t"]                # the points in the camera: the world frame becomes the camera's
    s["x3Dw"] = X.astype(np.float32); s["Tcw"] = np.eye(4, dtype=np.float32)
    s["x3Dw"][4] = (0.25, -0.5, 0.0)
    return s


def identical_points(n=12, stereo=False):
    """n times the same point and observation: every Jacobian is the same, H has rank 2 (3 with stereo)"""
    s = scene(41, n, "stereo" if stereo else "mono", outliers=0, noise=0.0)
    for k in ("x3Dw", "obs_xy", "u_right", "inv_sigma2"):
        s[k][:] = s[k][0]
    return s


def host():
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(ROOT, "sindslam_amd", "libsind_host.so"))
    return _host


class HostOptimizer:
    """sindh_pose_optimize with the interface of ORBmatcher.PoseOptimization (items -> list of result dicts)"""

    def __init__(self, K=K5):
        self.K = [C.c_float(float(k)) for k in K]

    def PoseOptimization(self, items):
        from sindslam_amd.matcher import poseopt_items, poseopt_result
        arr, keep = poseopt_items(items)
        rc = host().sindh_pose_optimize(arr, len(items), *self.K)
        assert rc == 0, rc
        return [poseopt_result(a) for a in keep]


def bits(a):
    """bit patterns, every NaN as one pattern (which NaN an operation returns decides nothing: no comparison with it holds)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return np.where(np.isnan(a), np.uint64(0x7ff8000000000000), a.view(np.uint64))
    if a.dtype == np.float32:
        return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))
    return a


def assert_same(got, ref, what):
    """every output of the call, as bit patterns; ref may be poseopt_ref's dict (Tcw / outlier None where n < 3: the input pose is then what `got` must still hold)"""
    for k in OUTPUTS:
        r = ref[k]
        if r is None:
            continue
        g = np.asarray(got[k]); r = np.asarray(r).astype(g.dtype) if np.asarray(r).dtype.kind in "iub" else np.asarray(r)
        assert g.shape == r.reshape(g.shape).shape and np.array_equal(bits(g), bits(r.reshape(g.shape))), (what, k, got[k], ref[k])
