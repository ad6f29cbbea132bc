"""Synthetic maps for sind_match_global_ba: key frames on an arc with banded co-visibility (every point is seen inside a sliding window of key frames) and optional loop
pairs, which give a block row of the reduced system whose envelope starts far to the left; a converter from a localba_scene.scene without fixed cameras; and the host
twin behind the interface of ORBmatcher.GlobalBundleAdjustment."""
import ctypes as C

import numpy as np

import localba_scene as SC
from localba_scene import K5, arc_pose, bits, project, rodrigues

OUTPUTS = ("Tcw", "x3Dw", "included", "n_iters", "chi2", "lambda_", "n_active_poses", "solver_fail", "env_entries", "env_dense_entries")
SIND_E_ARG, SIND_E_CAPACITY = -1, -5


def host():
    h = SC.host()
    h.sindh_global_ba.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    h.sindh_globalba_plan.argtypes = [C.c_void_p, C.c_void_p]
    h.sindh_globalba_linear.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    return h


class HostGBA:
    """sindh_global_ba with the interface of ORBmatcher.GlobalBundleAdjustment (items -> list of result dicts); rc: the expected return code"""

    def GlobalBundleAdjustment(self, items, iterations=10, robust=False, rc=0, K=K5):
        from sindslam_amd.matcher import globalba_items, globalba_result
        arr, keep = globalba_items(items)
        K = np.ascontiguousarray(K, np.float32)
        got = host().sindh_global_ba(arr, len(items), int(iterations), int(bool(robust)), K.ctypes.data)
        assert got == rc, (got, rc)
        return [globalba_result(a) for a in keep]


def assert_same(got, ref, what, keys=OUTPUTS):
    """every output of the call, as bit patterns"""
    for k in keys:
        g = np.asarray(got[k]); r = np.asarray(ref[k])
        r = r.astype(g.dtype) if r.dtype.kind in "iub" else r
        assert g.shape == r.reshape(g.shape).shape and np.array_equal(bits(g), bits(r.reshape(g.shape))), (what, k, got[k], ref[k])


def band_map(seed, n_kf, n_pts, window, obs_per_point, loops=(), kind="mixed", outliers=0, first_id=0, noise=0.5, start=(0.01, 0.03, 0.03), all_seen_by=None):
    """-> item (what ORBmatcher.GlobalBundleAdjustment takes) with truth_Tcw, truth_x3Dw and planted (u8 per observation) added.
    Key frames lie on arc_pose, ids first_id, first_id + 2, ... (first_id = 0: the first one is the fixed key frame of the map; > 0: nothing is fixed).  Every point is seen
    by obs_per_point key frames of a window of `window` consecutive ones, inserted in a shuffled order.  For each (a, b) in loops three more points are seen by key frames a
    and b alone.  all_seen_by: a key frame index that sees every point besides.  kind: mono, stereo or mixed (every third observation monocular).  outliers: how many
    observations (one per point, on points with at least 3) are displaced by 20 to 40 px.  Point ids are shuffled so that their order is not the item's."""
    rng = np.random.RandomState(seed)
    ang = np.linspace(-0.35, 0.35, n_kf) if n_kf > 1 else np.array([0.0])
    T = np.array([arc_pose(a) for a in ang])
    n_all = n_pts + 3 * len(loops)
    X = np.stack([rng.uniform(-2.0, 2.0, n_all), rng.uniform(-1.5, 1.5, n_all), rng.uniform(4.5, 7.5, n_all)], 1)
    kf_id = first_id + 2 * np.arange(n_kf)
    mp_id = rng.permutation(n_all) * 3 + 100
    obs_start, obs_kf, xy, ur, s2 = [0], [], [], [], []
    for j in range(n_all):
        if j < n_pts:
            w = min(window, n_kf); w0 = rng.randint(0, n_kf - w + 1)
            ks = w0 + rng.choice(w, min(obs_per_point, w), replace=False)
            if all_seen_by is not None and all_seen_by not in ks:
                ks = np.append(ks, all_seen_by)
        else:
            ks = np.array(loops[(j - n_pts) // 3])
        for k in rng.permutation(ks):
            u, v, r, _ = project(T[k], X[j])
            e = rng.normal(0, noise, 3) if noise else np.zeros(3)
            mono = kind == "mono" or (kind == "mixed" and len(obs_kf) % 3 == 0)
            obs_kf.append(int(k)); xy.append([u + e[0], v + e[1]]); ur.append(-1.0 if mono else r + e[2]); s2.append(1.0 / 1.2 ** (2 * rng.randint(0, 4)))
        obs_start.append(len(obs_kf))
    obs_start = np.array(obs_start, np.int32); xy = np.array(xy, np.float64).reshape(-1, 2); ur = np.array(ur, np.float64)
    planted = np.zeros(len(obs_kf), np.uint8)
    if outliers:
        ok = [j for j in range(n_all) if obs_start[j + 1] - obs_start[j] >= 3]
        for j in rng.choice(ok, min(outliers, len(ok)), replace=False):
            e = rng.randint(obs_start[j], obs_start[j + 1]); a = rng.uniform(0, 2 * np.pi)
            d = rng.uniform(20, 40) * np.array([np.cos(a), np.sin(a)])
            xy[e] += d; planted[e] = 1
            if ur[e] >= 0:
                ur[e] += d[0]
    T0 = T.copy()
    for k in range(n_kf):
        if kf_id[k] != 0:
            D = np.eye(4); D[:3, :3] = rodrigues(rng.normal(0, start[0], 3)); D[:3, 3] = rng.normal(0, start[1], 3)
            T0[k] = D @ T[k]
    X0 = X + rng.normal(0, start[2], X.shape)
    return dict(kf_id=kf_id.astype(np.int64), Tcw=T0.astype(np.float32), mp_id=mp_id.astype(np.int64), x3Dw=X0.astype(np.float32), obs_start=obs_start,
                obs_kf=np.array(obs_kf, np.int32), obs_xy=xy.astype(np.float32), u_right=ur.astype(np.float32), inv_sigma2=np.array(s2, np.float32),
                truth_Tcw=T, truth_x3Dw=X, planted=planted)


def from_local(s):
    """a localba_scene.scene without kind-2 cameras as a global-BA item: the key frames in ascending kf_id (kind 1 is the key frame with id 0, which both calls fix).
    -> item, order (item key frame k is the scene's key frame order[k])"""
    assert not np.any(np.asarray(s["kf_kind"]) == 2) and all((int(i) == 0) == (int(k) == 1) for i, k in zip(s["kf_id"], s["kf_kind"]))
    order = np.argsort(s["kf_id"], kind="stable"); inv = np.empty(len(order), np.int32); inv[order] = np.arange(len(order), dtype=np.int32)
    it = {k: s[k] for k in ("mp_id", "x3Dw", "obs_start", "obs_xy", "u_right", "inv_sigma2")}
    it.update(kf_id=np.asarray(s["kf_id"])[order], Tcw=np.asarray(s["Tcw"])[order], obs_kf=inv[np.asarray(s["obs_kf"], np.int64)] if len(s["obs_kf"]) else np.zeros(0, np.int32))
    return it, order


def without_point_obs(it, j):
    """a copy of the item in which point j has no observation"""
    a, b = int(it["obs_start"][j]), int(it["obs_start"][j + 1])
    out = dict(it)
    for k in ("obs_kf", "obs_xy", "u_right", "inv_sigma2", "planted"):
        if k in it:
            out[k] = np.concatenate([it[k][:a], it[k][b:]])
    st = np.array(it["obs_start"]).copy(); st[j + 1:] -= b - a; out["obs_start"] = st
    return out


def without_kf_obs(it, k):
    """a copy of the item in which key frame index k has no observation"""
    keep = np.asarray(it["obs_kf"]) != k
    out = dict(it)
    for key in ("obs_kf", "obs_xy", "u_right", "inv_sigma2", "planted"):
        if key in it:
            out[key] = it[key][keep]
    cs = np.concatenate([[0], np.cumsum(keep)]); out["obs_start"] = cs[np.asarray(it["obs_start"])].astype(np.int32)
    return out


def bad_items():
    """items that must be refused with SIND_E_ARG -> {name: item}"""
    b = band_map(15, 4, 8, 4, 3)
    cp = lambda **kw: dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}, **kw)
    out = {}
    a = cp(); a["kf_id"][1] = a["kf_id"][0]; out["kf ids repeat"] = a
    a = cp(); a["kf_id"][2] = a["kf_id"][1] - 1; out["kf ids descend"] = a
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
    return out
