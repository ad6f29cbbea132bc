"""Scenes for the Sim3Solver tests: two key frames that see the same points through two maps related by a known similarity (what a loop closure meets after
drift), pixel-scale noise, a share of gross outliers, octaves over all levels; and the same on two frames of the synthetic stream after SearchByBoW(KF, KF)."""
import numpy as np

K = (np.float32(535.4), np.float32(539.2), np.float32(320.1), np.float32(247.6))


def scale_factors():
    s = np.ones(8, np.float32)
    for i in range(1, 8):
        s[i] = np.float32(s[i - 1] * np.float32(1.2))                   # ORBextractor.cc:420-426
    return s


def sigma2_of(octave):
    s = scale_factors()
    return (s * s)[np.asarray(octave)]                                  # mvLevelSigma2 (ORBextractor.cc:425-431), FP32


def rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def pose(axis, angle, t):
    T = np.eye(4); T[:3, :3] = rot(axis, angle); T[:3, 3] = t
    return T


def candidate(seed, n, outliers=0.3, noise_px=0.5, s12=1.15, extra_slots=17, T2w=None):
    """-> the flattened Sim3Solver constructor (T1w, T2w, x3Dw1, x3Dw2, sigma2_1, sigma2_2, indices1, N1, K) and truth = (s12, R12, t12, is_outlier).
    Camera-frame points satisfy X1c = s12 R12 X2c + t12 up to the noise; an outlier's point in map 2 is somewhere else in the view.  T2w: pKF2's pose, if not the scene's own."""
    rng = np.random.default_rng(seed)
    T1w = pose((0.2, 1, 0.1), 0.3, (0.3, -0.1, 0.2)); T2w = pose((0.1, -1, 0.3), 0.2, (-0.4, 0.2, 0.1)) if T2w is None else np.asarray(T2w, np.float64)
    R12 = rot((0.3, 1, -0.2), 0.12); t12 = np.array([0.15, -0.05, 0.1])
    z = rng.uniform(1.0, 4.0, n); u = rng.uniform(20, 620, n); v = rng.uniform(20, 460, n)
    X1c = np.stack([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z], 1)
    X2c = (X1c - t12) @ R12 / s12                                       # R^T (x - t) / s
    X2c[:, :2] += rng.normal(0, noise_px, (n, 2)) * (X2c[:, 2:3] / float(K[0]))
    bad = rng.random(n) < outliers
    zb = rng.uniform(1.0, 4.0, n); ub = rng.uniform(20, 620, n); vb = rng.uniform(20, 460, n)
    X2c[bad] = np.stack([(ub - K[2]) * zb / K[0], (vb - K[3]) * zb / K[1], zb], 1)[bad]
    back = lambda T, X: (X - T[:3, 3]) @ T[:3, :3]                      # R^T (x - t)
    o1 = rng.integers(0, 8, n); o2 = np.clip(o1 + rng.integers(-1, 2, n), 0, 7)
    N1 = n + extra_slots
    inp = dict(T1w=T1w.astype(np.float32), T2w=T2w.astype(np.float32), x3Dw1=back(T1w, X1c).astype(np.float32), x3Dw2=back(T2w, X2c).astype(np.float32),
               sigma2_1=sigma2_of(o1), sigma2_2=sigma2_of(o2), indices1=np.sort(rng.choice(N1, n, replace=False)), N1=N1, K=K)
    return inp, (s12, R12, t12, bad)


def raw_values(seed, count=6000):
    """a list of rand() values"""
    return np.random.default_rng(seed).integers(0, 2 ** 31, count).tolist()


def rand_from(raw):
    it = iter(raw)
    return lambda: next(it)


def stream_candidate(stream, t1, t2, match12, drift=1.08):
    """Frames t1 and t2 of the synthetic stream as pKF1 / pKF2 after SearchByBoW(pKF1, pKF2) gave match12: every keypoint's map point is its depth back-projected with the
    ground-truth pose; map 2 and pKF2's pose have drifted by the scale `drift` (camera-2 coordinates are `drift` times the true ones, so s12 is about 1 / drift).  Wrong
    descriptor matches are the outliers."""
    import bow_scene as B
    f1, f2 = B.stream_frame(stream, t1), B.stream_frame(stream, t2)
    cam = f1["cam"]

    def world(f, k):
        z = f["depth"][k].astype(np.float64); xy = f["un_xy"][k].astype(np.float64)
        Xc = np.stack([(xy[:, 0] - cam[2]) * z / cam[0], (xy[:, 1] - cam[3]) * z / cam[1], z], 1)
        T = f["Tcw"].astype(np.float64)
        return (Xc - T[:3, 3]) @ T[:3, :3]
    i1 = np.nonzero(match12 >= 0)[0]; i2 = match12[i1]
    T2 = f2["Tcw"].astype(np.float64).copy(); T2[:3, 3] *= drift
    return dict(T1w=f1["Tcw"], T2w=T2.astype(np.float32), x3Dw1=world(f1, i1).astype(np.float32), x3Dw2=(drift * world(f2, i2)).astype(np.float32),
                sigma2_1=sigma2_of(f1["octave"][i1]), sigma2_2=sigma2_of(f2["octave"][i2]), indices1=i1, N1=len(match12), K=tuple(np.float32(c) for c in cam[:4]))
