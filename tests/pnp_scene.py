"""Relocalisation candidates for the PnP tests: map points in front of a ground-truth camera, their projections with pixel noise, and an outlier share (a float)
or number (an int) whose image points are drawn anew.  A candidate is the flattened PnPsolver constructor (include/sind_hip.h, sind_pnp_item)."""
from __future__ import annotations

import numpy as np

K = (535.4, 539.2, 320.1, 247.6)                                      # fx fy cx cy (TUM3)
SIGMA2 = np.float32(1.2) ** (2 * np.arange(8, dtype=np.float32))      # mvLevelSigma2 of 8 levels at scale 1.2


def pose(rng, angle=0.4, shift=0.5):
    """a ground-truth [R | t]: a rotation by up to `angle` about a random axis, a translation of up to `shift`"""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax); a = rng.uniform(-angle, angle)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    return R, rng.uniform(-shift, shift, 3)


def candidate(seed, n, outliers=0.3, noise=0.5, n_keypoints=None, th2=5.991):
    """-> dict: x3Dw f32 [n, 3], p2d f32 [n, 2], sigma2 f32 [n], th2, indices (mvKeyPointIndices, ascending) i64 [n], n_keypoints, and the truth R, t, is_outlier; key names the candidate"""
    rng = np.random.default_rng(seed)
    R, t = pose(rng)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 8, n)], 1)
    Xw = (Xc - t) @ R                                                   # R^T (Xc - t)
    Xw = Xw.astype(np.float32)
    Xc = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([K[2] + K[0] * Xc[:, 0] / Xc[:, 2], K[3] + K[1] * Xc[:, 1] / Xc[:, 2]], 1) + rng.normal(0, noise, (n, 2)) * (noise > 0)
    if isinstance(outliers, int):                                       # exactly that many
        out = np.zeros(n, bool); out[rng.choice(n, outliers, replace=False)] = True
    else:
        out = rng.random(n) < outliers
    uv[out] = np.stack([rng.uniform(0, 640, out.sum()), rng.uniform(0, 480, out.sum())], 1)
    n_keypoints = n_keypoints or 2 * n + 3
    idx = np.sort(rng.choice(n_keypoints, n, replace=False))
    return dict(x3Dw=Xw, p2d=uv.astype(np.float32), sigma2=SIGMA2[rng.integers(0, 8, n)].astype(np.float32), th2=float(np.float32(th2)), indices=idx.astype(np.int64), n_keypoints=int(n_keypoints),
                R=R, t=t, is_outlier=out, key=(seed, n, outliers, noise, n_keypoints, th2))


def rand_stream(seed):
    """a stand-in for glibc's rand(): raw values in [0, RAND_MAX]"""
    rng = np.random.default_rng(seed)
    return lambda: int(rng.integers(0, 2147483648))


def stream_candidate(stream, t_kf, t_cur, match_of_cur, valid, ideal_map=False):
    """Frame t_cur of the synthetic stream as the lost frame and frame t_kf as a candidate key frame after SearchByBoW(pKF, F) gave match_of_cur: the flattened PnPsolver
    constructor.  A key-frame keypoint's map point is its depth back-projected with the ground-truth pose; wrong descriptor matches are the outliers.
    ideal_map: the map is as exact as the scenes of `candidate` without noise are.  A map point whose match is right (under the frame's ground-truth pose it projects
    within the bound CheckInliers uses, 5.991 sigma2) is moved, at its depth in the frame's camera, onto the ray of the frame's keypoint, so its projection is the
    keypoint up to the FP32 rounding of the point; a map point whose match is wrong stays where it is and stays an outlier.  The ground-truth pose is then recoverable to
    the precision of the arithmetic, which is what the chain test asks of the pose it ends with."""
    import bow_scene as B
    import sim3_scene as S3
    kf, cur = B.stream_frame(stream, t_kf), B.stream_frame(stream, t_cur)
    cam = kf["cam"]
    i = np.nonzero(match_of_cur >= 0)[0]; k = match_of_cur[i]
    assert valid[k].all()
    z = kf["depth"][k].astype(np.float64); xy = kf["un_xy"][k].astype(np.float64)
    Xc = np.stack([(xy[:, 0] - cam[2]) * z / cam[0], (xy[:, 1] - cam[3]) * z / cam[1], z], 1)
    T = kf["Tcw"].astype(np.float64)
    Xw = (Xc - T[:3, 3]) @ T[:3, :3]
    p2d = cur["un_xy"][i].astype(np.float32); sigma2 = S3.sigma2_of(cur["octave"][i]).astype(np.float32)
    right = np.zeros(len(i), bool)
    if ideal_map:
        Tc = cur["Tcw"].astype(np.float64); fx, fy, cx, cy = (float(c) for c in cam[:4])
        Pc = Xw @ Tc[:3, :3].T + Tc[:3, 3]
        with np.errstate(all="ignore"):
            e2 = (cx + fx * Pc[:, 0] / Pc[:, 2] - p2d[:, 0]) ** 2 + (cy + fy * Pc[:, 1] / Pc[:, 2] - p2d[:, 1]) ** 2
        right = (Pc[:, 2] > 0) & (e2 < 5.991 * sigma2)
        zc = Pc[right, 2]; u = p2d[right].astype(np.float64)
        Xw[right] = (np.stack([(u[:, 0] - cx) * zc / fx, (u[:, 1] - cy) * zc / fy, zc], 1) - Tc[:3, 3]) @ Tc[:3, :3]
    return dict(x3Dw=Xw.astype(np.float32), p2d=p2d, sigma2=sigma2, th2=float(np.float32(5.991)), indices=i.astype(np.int64), n_keypoints=len(match_of_cur),
                key=("stream", t_kf, t_cur, ideal_map), right=right)
