"""A synthetic local window for sind_match_local_ba: key frames on an arc that look at a point cloud, pixel noise, monocular, stereo or mixed observations, planted
outliers, perturbed poses and points; the host twin behind the interface of ORBmatcher.LocalBundleAdjustment; and a small map of plain dicts for
sindslam_amd.optimizer.LocalBundleAdjustment."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K5 = np.array([520.0, 516.0, 320.0, 240.0, 40.0], np.float32)          # fx fy cx cy bf
OUTPUTS = ("Tcw", "x3Dw", "erase", "n_stages", "n_level1", "stage_iters", "stage_chi2", "stage_lambda")
_host = None


def host():
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(ROOT, "sindslam_amd", "libsind_host.so"))
        _host.sindh_local_ba.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return _host


class HostBA:
    """sindh_local_ba with the interface of ORBmatcher.LocalBundleAdjustment (items -> list of result dicts); rc: the expected return code"""

    def LocalBundleAdjustment(self, items, rc=0, K=K5):
        from sindslam_amd.matcher import localba_items, localba_result
        arr, keep = localba_items(items)
        K = np.ascontiguousarray(K, np.float32)
        got = host().sindh_local_ba(arr, len(items), K.ctypes.data)
        assert got == rc, (got, rc)
        return [localba_result(a) for a in keep]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same(got, ref, what):
    """every output of the call, as bit patterns"""
    for k in OUTPUTS:
        g = np.asarray(got[k]); r = np.asarray(ref[k])
        r = r.astype(g.dtype) if r.dtype.kind in "iub" else r
        assert g.shape == r.reshape(g.shape).shape and np.array_equal(bits(g), bits(r.reshape(g.shape))), (what, k, got[k], ref[k])


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def arc_pose(a, radius=6.0):
    """Tcw of a camera on a circle of `radius` around (0, 0, radius) at angle a, looking at the centre"""
    R = rodrigues([0.0, -a, 0.0])                                     # camera to world
    c = np.array([0.0, 0.0, radius]) - R @ np.array([0.0, 0.0, radius])
    T = np.eye(4); T[:3, :3] = R.T; T[:3, 3] = -R.T @ c
    return T


def project(T, X, K=K5):
    p = T[:3, :3] @ X + T[:3, 3]
    u = float(K[0]) * p[0] / p[2] + float(K[2]); v = float(K[1]) * p[1] / p[2] + float(K[3])
    return u, v, u - float(K[4]) / p[2], p[2]


def scene(seed, n_local=4, n_fixed=1, n_pts=30, kind="mixed", noise=0.5, outliers=0, start=(0.01, 0.03, 0.03), obs_per_point=None, id0=False, first_id=3):
    """-> item (what ORBmatcher.LocalBundleAdjustment takes) with truth_Tcw, truth_x3Dw, planted (u8 per observation) added.
    kind: mono, stereo or mixed (every third observation monocular).  outliers: how many observations (on points with at least 3, at most one per point) are displaced by 20 to 40 px.
    start: the perturbation of the free poses (rad, m) and of the points (m).  obs_per_point: None = every key frame sees every point, else that many, chosen per point.
    id0: the first local key frame has id 0 and kind 1.  Key-frame and point ids are shuffled so that neither order is the item's."""
    rng = np.random.RandomState(seed)
    n_kf = n_local + n_fixed
    ang = np.linspace(-0.35, 0.35, n_kf) if n_kf > 1 else np.array([0.0])
    T = np.array([arc_pose(a) for a in rng.permutation(ang)])
    X = np.stack([rng.uniform(-2.0, 2.0, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4.5, 7.5, n_pts)], 1)
    kf_id = rng.permutation(n_kf) * 2 + first_id
    kind_kf = np.array([0] * n_local + [2] * n_fixed, np.uint8)
    if id0:
        kf_id[0] = 0; kind_kf[0] = 1
    mp_id = rng.permutation(n_pts) * 3 + 100
    obs_start, obs_kf, xy, ur, s2 = [0], [], [], [], []
    for j in range(n_pts):
        ks = np.arange(n_kf) if obs_per_point is None else np.sort(rng.choice(n_kf, min(obs_per_point, n_kf), replace=False))
        for k in rng.permutation(ks):
            u, v, r, _ = project(T[k], X[j])
            lvl = rng.randint(0, 4)
            e = rng.normal(0, noise, 3) if noise else np.zeros(3)
            mono = kind == "mono" or (kind == "mixed" and len(obs_kf) % 3 == 0)
            obs_kf.append(k); xy.append([u + e[0], v + e[1]]); ur.append(-1.0 if mono else r + e[2]); s2.append(1.0 / 1.2 ** (2 * lvl))
        obs_start.append(len(obs_kf))
    obs_start = np.array(obs_start, np.int32); xy = np.array(xy, np.float64).reshape(-1, 2); ur = np.array(ur, np.float64)
    planted = np.zeros(len(obs_kf), np.uint8)
    if outliers:
        ok = [j for j in range(n_pts) if obs_start[j + 1] - obs_start[j] >= 3]                     # at most one per point
        for j in rng.choice(ok, min(outliers, len(ok)), replace=False):
            e = rng.randint(obs_start[j], obs_start[j + 1])
            d = rng.uniform(20, 40) * np.array([np.cos(a := rng.uniform(0, 2 * np.pi)), np.sin(a)])
            xy[e] += d; planted[e] = 1
            if ur[e] >= 0:
                ur[e] += d[0]
    T0 = T.copy()
    for k in range(n_kf):
        if kind_kf[k] == 0:
            D = np.eye(4); D[:3, :3] = rodrigues(rng.normal(0, start[0], 3)); D[:3, 3] = rng.normal(0, start[1], 3)
            T0[k] = D @ T[k]
    X0 = X + rng.normal(0, start[2], X.shape)
    return dict(kf_id=kf_id.astype(np.int64), kf_kind=kind_kf, Tcw=T0.astype(np.float32), mp_id=mp_id.astype(np.int64), x3Dw=X0.astype(np.float32), obs_start=obs_start,
                obs_kf=np.array(obs_kf, np.int32), obs_xy=xy.astype(np.float32), u_right=ur.astype(np.float32), inv_sigma2=np.array(s2, np.float32), do_more=True,
                truth_Tcw=T, truth_x3Dw=X, planted=planted)


def mean_reprojection_error(Tcw, x3Dw, item, keep):
    """the mean pixel distance of the kept observations from the projections (u and v only)"""
    d = []
    for j in range(len(item["mp_id"])):
        for e in range(item["obs_start"][j], item["obs_start"][j + 1]):
            if keep[e]:
                u, v, _, _ = project(np.asarray(Tcw[item["obs_kf"][e]], np.float64), np.asarray(x3Dw[j], np.float64))
                d.append(np.hypot(u - item["obs_xy"][e, 0], v - item["obs_xy"][e, 1]))
    return float(np.mean(d))


def toy_map(seed, n_kf=6, n_pts=150, outliers=0.05, noise=0.5, start=(0.01, 0.03, 0.03), share=0.85, min_obs=5, levels=1):
    """A map of plain dicts for optimizer.LocalBundleAdjustment: n_kf key frames (ids 0 .. n_kf - 1; 0 is the first of the map and fixed), each seeing a random `share` of
    the points on one of `levels` pyramid levels, stereo and monocular slots mixed; the planted outliers (20 to 40 px) sit on points with at least min_obs observations, one per point,
    and point up or down within 0.5 rad: the key frames lie on a horizontal arc, where a horizontal displacement in an end camera is nearly a change of depth, which the
    five robust iterations of the first stage do not resolve, so that a neighbour's good observation goes to level 1 with it; covisibility from the shared observations, most first.  -> keyframes, mappoints, planted = set of (kf id, mp id)"""
    rng = np.random.RandomState(seed)
    T = [arc_pose(a) for a in np.linspace(-0.35, 0.35, n_kf)]
    X = np.stack([rng.uniform(-2.0, 2.0, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4.5, 7.5, n_pts)], 1)
    keyframes, mappoints, planted = {}, {m: dict(x3Dw=(X[m] + rng.normal(0, start[2], 3)).astype(np.float32), obs={}, bad=False) for m in range(n_pts)}, set()
    for k in range(n_kf):
        see = np.sort(rng.choice(n_pts, int(share * n_pts), replace=False)); n = len(see)
        xy = np.zeros((n, 2)); ur = np.zeros(n); s2 = np.zeros(n)
        for sl, m in enumerate(see):
            u, v, r, _ = project(T[k], X[m]); e = rng.normal(0, noise, 3)
            xy[sl] = [u + e[0], v + e[1]]; ur[sl] = -1.0 if (sl + k) % 3 == 0 else r + e[2]; s2[sl] = 1.0 / 1.2 ** (2 * rng.randint(0, levels))
            mappoints[m]["obs"][k] = sl
        D = np.eye(4)
        if k:
            D[:3, :3] = rodrigues(rng.normal(0, start[0], 3)); D[:3, 3] = rng.normal(0, start[1], 3)
        keyframes[k] = dict(Tcw=(D @ T[k]).astype(np.float32), un_xy=xy, u_right=ur, inv_sigma2=s2.astype(np.float32), mp=see.astype(np.int64), bad=False)
    cand = [m for m in range(n_pts) if len(mappoints[m]["obs"]) >= min_obs]
    for m in rng.choice(cand, int(outliers * sum(len(p["obs"]) for p in mappoints.values())), replace=False):
        k = sorted(mappoints[m]["obs"])[rng.randint(len(mappoints[m]["obs"]))]; sl = mappoints[m]["obs"][k]
        a = rng.choice([0.5, 1.5]) * np.pi + rng.uniform(-0.5, 0.5); d = rng.uniform(20, 40) * np.array([np.cos(a), np.sin(a)])      # within 0.5 rad of the vertical, see above
        keyframes[k]["un_xy"][sl] += d
        if keyframes[k]["u_right"][sl] >= 0:
            keyframes[k]["u_right"][sl] += d[0]
        planted.add((k, m))
    for k in range(n_kf):
        w = {q: len(set(keyframes[k]["mp"].tolist()) & set(keyframes[q]["mp"].tolist())) for q in range(n_kf) if q != k}
        keyframes[k]["covisible"] = sorted(w, key=lambda q: (-w[q], q))
        keyframes[k]["un_xy"] = keyframes[k]["un_xy"].astype(np.float32); keyframes[k]["u_right"] = keyframes[k]["u_right"].astype(np.float32)
    return keyframes, mappoints, planted


def with_point(item, X, obs, mp_id=None):
    """a copy of the item with one more point at X (the last in the item) and its observations [(key frame index, x, y, u_right, inv_sigma2)]"""
    it = dict(item)
    it["mp_id"] = np.append(item["mp_id"], (int(item["mp_id"].max()) + 7 if len(item["mp_id"]) else 5) if mp_id is None else mp_id).astype(np.int64)
    it["x3Dw"] = np.concatenate([item["x3Dw"], np.array([X], np.float32)]).astype(np.float32)
    it["obs_start"] = np.append(item["obs_start"], item["obs_start"][-1] + len(obs)).astype(np.int32)
    it["obs_kf"] = np.append(item["obs_kf"], [o[0] for o in obs]).astype(np.int32)
    it["obs_xy"] = np.concatenate([item["obs_xy"], np.array([[o[1], o[2]] for o in obs], np.float32).reshape(-1, 2)]).astype(np.float32)
    it["u_right"] = np.append(item["u_right"], [o[3] for o in obs]).astype(np.float32)
    it["inv_sigma2"] = np.append(item["inv_sigma2"], [o[4] for o in obs]).astype(np.float32)
    it["planted"] = np.append(item["planted"], np.zeros(len(obs), np.uint8))
    return it


def seen(item, k, X, dxy=(0.0, 0.0), mono=True):
    """the observation of X in key frame index k at the item's true pose, displaced by dxy"""
    u, v, r, _ = project(item["truth_Tcw"][k], np.asarray(X, np.float64))
    return (k, u + dxy[0], v + dxy[1], -1.0 if mono else r + dxy[0], 1.0)


def literal_cases():
    """the literal and degenerate cases of the issue -> {name: item}"""
    base = scene(11, 3, 1, 14, kind="mixed")
    out = {}
    X = np.array([0.3, -0.2, 6.0])
    out["single_mono"] = with_point(base, X, [seen(base, 0, X)])                                   # Hll is invertible only through lambda
    out["point_all_level1"] = with_point(base, X, [seen(base, 0, X, (90.0, 0.0)), seen(base, 1, X, (0.0, -90.0)), seen(base, 3, X, (-90.0, 60.0), mono=False)])
    few = scene(12, 3, 1, 14, kind="mixed")
    k = 2; rng = np.random.RandomState(5)                                # every observation of local key frame 2 is pushed 150 to 250 px away, each its own way
    few["obs_xy"] = few["obs_xy"].copy(); few["u_right"] = few["u_right"].copy()
    few["inv_sigma2"] = np.ones_like(few["inv_sigma2"])                  # one pyramid level: a displaced observation does not outweigh the three honest ones of its point
    for i, e in enumerate(np.nonzero(few["obs_kf"] == k)[0]):
        a = rng.uniform(0, 2 * np.pi); d = (rng.uniform(150, 250) * np.array([np.cos(a), np.sin(a)])).astype(np.float32)      # no pose of the key frame fits fourteen of these
        few["obs_xy"][e] += d
        if few["u_right"][e] >= 0:
            few["u_right"][e] += d[0]
    out["kf_all_level1"] = few
    out["id0"] = scene(13, 3, 1, 14, kind="mixed", id0=True)
    Xb = np.linalg.inv(base["truth_Tcw"][1]) @ np.array([0.2, 0.1, -3.0, 1.0])                     # behind key frame 1
    out["behind"] = with_point(base, Xb[:3], [seen(base, 0, Xb[:3]), seen(base, 1, Xb[:3]), seen(base, 2, Xb[:3])])      # seen where it projects: only the depth speaks
    z0 = dict(base); z0["Tcw"] = base["Tcw"].copy(); z0["Tcw"][3] = np.eye(4, dtype=np.float32)    # the fixed camera at the identity, the point in its plane z = 0
    out["depth0"] = with_point(z0, [0.5, 0.25, 0.0], [(3, 300.0, 200.0, -1.0, 1.0), seen(base, 0, X), seen(base, 1, X)])
    out["depth0_stop"] = dict(out["depth0"], do_more=False)
    out["do_more0"] = dict(scene(14, 3, 1, 14, kind="mixed", outliers=3), do_more=False)
    e = dict(base)
    e.update(obs_start=np.zeros(len(base["mp_id"]) + 1, np.int32), obs_kf=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32), u_right=np.zeros(0, np.float32), inv_sigma2=np.zeros(0, np.float32),
             planted=np.zeros(0, np.uint8))
    out["n_obs0"] = e
    p = dict(e); p.update(mp_id=np.zeros(0, np.int64), x3Dw=np.zeros((0, 3), np.float32), obs_start=np.zeros(1, np.int32))
    out["n_mp0"] = p
    return out


def bad_items():
    """items that must be refused with SIND_E_ARG -> {name: item}"""
    b = scene(15, 3, 1, 8, kind="mixed")
    cp = lambda **kw: dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}, **kw)
    out = {}
    a = cp(); a["kf_id"][1] = a["kf_id"][0]; out["kf ids repeat"] = a
    a = cp(); a["mp_id"][3] = a["mp_id"][5]; out["mp ids repeat"] = a
    a = cp(); a["obs_kf"][2] = 4; out["obs_kf too large"] = a
    a = cp(); a["obs_kf"][2] = -1; out["obs_kf negative"] = a
    a = cp(); a["obs_kf"][1] = a["obs_kf"][0]; out["a key frame twice in a point"] = a
    a = cp(); a["obs_start"][2] = a["obs_start"][3] + 1; out["obs_start decreases"] = a
    a = cp(); a["obs_start"][0] = 1; out["obs_start does not start at 0"] = a
    a = cp(); a["inv_sigma2"][4] = -1.0; out["negative inv_sigma2"] = a
    a = cp(); a["inv_sigma2"][4] = np.inf; out["infinite inv_sigma2"] = a
    a = cp(); a["Tcw"][1, 0, 3] = np.nan; out["pose not finite"] = a
    a = cp(); a["x3Dw"][2, 1] = np.inf; out["point not finite"] = a
    a = cp(); a["kf_kind"][:] = 2; out["no key frame of kind 0"] = a
    a = cp(); a["kf_kind"][1] = 3; out["kind outside 0..2"] = a
    return out
