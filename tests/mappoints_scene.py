"""Scenes for sind_match_triangulate and sind_match_update_points: two key frames that look at a point cloud with pixel noise, monocular, stereo or mixed keypoints and
some wrong matches; the literal cases, each built so that exactly one test of the loop rejects the match; lists of map points with their observations; the host twins
behind the interface of ORBmatcher.Triangulate / UpdateMapPoints; and a small map of plain dicts for sindslam_amd.mapping."""
import ctypes as C
import os

import numpy as np

import localba_scene as LS
import mappoints_ref as R
import sim3_scene as S3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K5 = np.array([520.0, 516.0, 320.0, 240.0, 40.0], np.float32)          # fx fy cx cy bf: mb = 0.0769 m
SCALE = S3.scale_factors()                                             # 8 levels, 1.2 apart
TRI_OUT = ("x3D", "how", "status", "nnew")
MP_OUT = ("desc", "best_obs", "normal", "max_dist", "min_dist", "updated")
f32 = np.float32
_host = None


def host():
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(ROOT, "sindslam_amd", "libsind_host.so"))
        _host.sindh_triangulate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        _host.sindh_update_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return _host


class HostMap:
    """sindh_triangulate and sindh_update_points with the interface of ORBmatcher (items -> list of result dicts); rc: the expected return code.  SearchForTriangulation is
    the Python restatement of bow_ref, so that sindslam_amd.mapping runs without a GPU."""
    K5 = tuple(float(v) for v in K5)
    checkOri = False

    def Triangulate(self, pairs, rc=0):
        from sindslam_amd.matcher import triangulate_items, triangulate_result
        arr, keep = triangulate_items(pairs)
        got = host().sindh_triangulate(arr, len(pairs), K5.ctypes.data, SCALE.ctypes.data, len(SCALE))
        assert got == rc, (got, rc)
        return [triangulate_result(a) for a in keep]

    def UpdateMapPoints(self, items, rc=0):
        from sindslam_amd.matcher import mappoints_items, mappoints_result
        arr, keep = mappoints_items(items)
        got = host().sindh_update_points(arr, len(items), SCALE.ctypes.data, len(SCALE))
        assert got == rc, (got, rc)
        return [mappoints_result(a) for a in keep]

    def SearchForTriangulation(self, pairs, bOnlyStereo=False):
        import bow_ref as W
        cam = np.array([*K5, K5[4] / K5[0], 0, 640, 0, 480], np.float32)
        out = []
        for T2, Cw1, F12, k1, k2 in pairs:
            m, n, p = W.search_for_triangulation(cam, SCALE, T2, Cw1, F12, k1, k2, bOnlyStereo, self.checkOri)
            out.append((m, n, np.array(p, np.int64).reshape(-1, 2)))
        return out


def assert_same(got, ref, keys, what):
    """every output of the call, as bit patterns"""
    for k in keys:
        g = np.asarray(got[k]); r = np.asarray(ref[k])
        r = r.astype(g.dtype) if r.dtype.kind in "iub" else r
        assert g.shape == r.reshape(g.shape).shape and np.array_equal(LS.bits(g), LS.bits(r.reshape(g.shape))), (what, k, got[k], ref[k])


def poses(Rwc, c):
    """-> Tcw, Twc as float32 [4, 4]: camera-to-world rotation Rwc and centre c; Twc in float from Tcw, as SetPose forms it"""
    T = np.eye(4); T[:3, :3] = Rwc.T; T[:3, 3] = -Rwc.T @ c
    T = T.astype(np.float32)
    W = np.eye(4, dtype=np.float32); W[:3, :3] = T[:3, :3].T; W[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return T, W


def _project(T, X):
    p = np.asarray(T, np.float64)[:3, :3] @ X + np.asarray(T, np.float64)[:3, 3]
    return float(K5[0]) * p[0] / p[2] + float(K5[2]), float(K5[1]) * p[1] / p[2] + float(K5[3]), p[2]


def tri_scene(seed, n, kind="mixed", baseline=None, noise=0.5, wrong=0.08, unmatched=0.1, extra=5, depth=(1.0, 4.0)):
    """-> the dict ORBmatcher.Triangulate takes.  n keypoints in key frame 1, n + extra in key frame 2 in another order; a share `unmatched` of match12 is -1 and a share
    `wrong` points at a random keypoint.  kind: mono, stereo or mixed (every keypoint stereo with probability 1 / 2).  baseline: metres, None = 0.1 .. 0.5 by the seed"""
    rng = np.random.RandomState(seed)
    b = rng.uniform(0.1, 0.5) if baseline is None else baseline
    R1 = LS.rodrigues(rng.normal(0, 0.1, 3)); c1 = rng.normal(0, 0.2, 3)
    R2 = R1 @ LS.rodrigues(rng.normal(0, 0.03, 3)); c2 = c1 + R1 @ np.array([b, rng.normal(0, 0.02), rng.normal(0, 0.02)])
    T1, W1 = poses(R1, c1); T2, W2 = poses(R2, c2)
    z = rng.uniform(depth[0], depth[1], n); u = rng.uniform(40, 600, n); v = rng.uniform(40, 440, n)
    X = (R1 @ np.stack([(u - K5[2]) * z / K5[0], (v - K5[3]) * z / K5[1], z])).T + c1
    n2 = n + extra; perm = rng.permutation(n2)

    def side(T, count, src):
        un = np.zeros((count, 2)); ur = np.full(count, -1.0); dp = np.full(count, -1.0)
        for i in range(count):
            uu, vv, zz = _project(T, X[src[i]]) if src[i] >= 0 else (rng.uniform(40, 600), rng.uniform(40, 440), rng.uniform(1, 4))
            e = rng.normal(0, noise, 3) if noise else np.zeros(3)
            un[i] = (uu + e[0], vv + e[1])
            if kind == "stereo" or (kind == "mixed" and rng.rand() < 0.5):
                ur[i] = uu - float(K5[4]) / zz + e[2]; dp[i] = abs(zz) * (1 + rng.normal(0, 0.002))
        return un, ur, dp

    un1, ur1, dp1 = side(T1, n, np.arange(n))
    src2 = np.full(n2, -1); src2[perm[:n]] = np.arange(n)
    un2, ur2, dp2 = side(T2, n2, src2)
    oct1 = rng.randint(0, 8, n); oct2 = rng.randint(0, 8, n2); oct2[perm[:n]] = np.where(rng.rand(n) < 0.85, oct1, oct2[perm[:n]])
    m12 = perm[:n].astype(np.int32)
    bad = rng.rand(n); m12[bad < wrong] = rng.randint(0, n2, int((bad < wrong).sum())); m12[bad > 1 - unmatched] = -1
    mk = lambda un, ur, dp, oc: dict(xy=(un + np.array([0.3, -0.2])).astype(f32), un_xy=un.astype(f32), octave=oc.astype(np.int32), u_right=ur.astype(f32), depth=dp.astype(f32))
    return dict(Tcw1=T1, Twc1=W1, Tcw2=T2, Twc2=W2, kf1=mk(un1, ur1, dp1, oct1), kf2=mk(un2, ur2, dp2, oct2), match12=m12)


def one_match(X, b, stereo1=False, stereo2=False, T2=None, oct1=0, oct2=0):
    """one pair with one match: camera 1 at the origin, camera 2 at (b, 0, 0) with the same orientation (or the pose T2 = (Rwc, centre)); the keypoints are the exact
    projections of X, stereo sides with u_right = u - bf / z and depth = z"""
    T1, W1 = poses(np.eye(3), np.zeros(3)); T2, W2 = poses(*(T2 if T2 is not None else (np.eye(3), np.array([b, 0.0, 0.0]))))
    X = np.asarray(X, np.float64)

    def side(T, stereo, octave):
        u, v, z = _project(T, X)
        return dict(xy=np.array([[u, v]], f32), un_xy=np.array([[u, v]], f32), octave=np.array([octave], np.int32), u_right=np.array([u - float(K5[4]) / z if stereo else -1.0], f32),
                    depth=np.array([z if stereo else -1.0], f32))
    return dict(Tcw1=T1, Twc1=W1, Tcw2=T2, Twc2=W2, kf1=side(T1, stereo1, oct1), kf2=side(T2, stereo2, oct2), match12=np.array([0], np.int32))


def cos_rays(pair):
    """cosParallaxRays of the one match of a pair, as the library forms it"""
    c = R.camera(K5, SCALE)
    T = lambda k: [[f32(v) for v in row] for row in np.asarray(pair[k], f32)]
    return R.cos_parallax_rays(c, T("Tcw1"), T("Tcw2"), pair["kf1"]["un_xy"][0], pair["kf2"]["un_xy"][int(pair["match12"][0])])


def tri_literal_cases():
    """-> {name: (pair, status, how)}: one match each, built so that the named test is the ONLY one that rejects it (or none does)"""
    X = np.array([0.2, 0.1, 2.0]); near = 0.01                          # 0.3 m: rays 0.15 rad apart; 0.01 m: 0.005 rad, cos above every stereo cosine at 2 m (0.99926)
    out = {}
    out["new_mono"] = (one_match(X, 0.3), 0, 0)
    out["stereo1_triangulated"] = (one_match(X, 0.3, True, False), 0, 0)       # cosParallaxRays < cosParallaxStereo1
    out["stereo1_unprojected"] = (one_match(X, near, True, False), 0, 1)       # the ordering the other way
    out["stereo2_triangulated"] = (one_match(X, 0.3, False, True), 0, 0)
    out["stereo2_unprojected"] = (one_match(X, near, False, True), 0, 2)
    out["stereo_both_triangulated"] = (one_match(X, 0.3, True, True), 0, 0)
    out["stereo_both_unprojected"] = (one_match(X, near, True, True), 0, 1)    # cosParallaxStereo2 is never formed when side 1 is stereo: always key frame 1
    out["low_parallax_mono"] = (one_match(X, near), 1, -1)
    lo, hi = 0.030, 0.050                                               # the baseline at which the FP32 cosParallaxRays crosses 0.9998, by bisection on the library's own value
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if np.float64(cos_rays(one_match(X, mid))) < 0.9998: hi = mid
        else: lo = mid
    out["cos_just_below_0.9998"] = (one_match(X, hi), 0, 0)
    out["cos_just_above_0.9998"] = (one_match(X, lo), 1, -1)
    # w == 0: both keys at the principal point, so A = -(rows 0 and 1 of both poses), and the poses (finite is all the call asks) chosen so that A's columns are orthogonal
    # with a zero third one: no rotation happens, the sort moves e3 to the last row, x3D = (0, 0, 1, 0).  Rows 2 give the rays (0, 0, 1) and (0.1, 0, 1): cos = 0.995
    p = one_match(X, 0.3)
    p["Tcw2"] = np.array([[0, 0, 0, 1], [0, 0, 0, 0], [0.1, 0, 1, 0], [0, 0, 0, 1]], f32)
    for k in ("kf1", "kf2"):
        p[k]["un_xy"] = np.array([[K5[2], K5[3]]], f32); p[k]["xy"] = p[k]["un_xy"].copy()
    out["w0"] = (p, 2, 0)
    out["behind_both"] = (one_match([0.2, 0.1, -2.0], 0.3), 3, 0)
    # behind camera 2 only: camera 2 ahead of the point, looking the same way; its key is where the line through the point meets its image, so the rays meet at the point
    out["behind_camera2_triangulated"] = (one_match([0.0, 0.0, 2.0], 0.0, T2=(np.eye(3), np.array([0.3, 0.0, 4.0]))), 4, 0)
    # and by UnprojectStereo of key frame 1: camera 2 looks along +x from (1, 0, 2), its key at the principal point: the rays are perpendicular (cos = 0, not > 0)
    Ry = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    p = one_match([0.0, 0.0, 2.0], 0.0, True, False, T2=(Ry, np.array([1.0, 0.0, 2.0])))
    p["kf2"]["un_xy"] = np.array([[K5[2], K5[3]]], f32); p["kf2"]["xy"] = p["kf2"]["un_xy"].copy()
    out["behind_camera2_unprojected"] = (p, 4, 1)
    p = one_match(X, near, False, True); p["kf1"]["un_xy"][0, 1] += 12.0      # the point is key frame 2's own unprojection: only key frame 1 (mono, 5.991) disagrees
    out["reprojection1_mono"] = (p, 5, 2)
    p = one_match(X, 0.3, True, True); p["kf1"]["u_right"][0] += 12.0          # triangulated from the two keys, which agree: only u_right of key frame 1 (7.8) disagrees
    out["reprojection1_stereo"] = (p, 5, 0)
    p = one_match(X, near, True, False); p["kf2"]["un_xy"][0, 1] += 12.0
    out["reprojection2_mono"] = (p, 6, 1)
    p = one_match(X, 0.3, True, True); p["kf2"]["u_right"][0] += 12.0
    out["reprojection2_stereo"] = (p, 6, 0)
    # a zero distance: the point is key frame 1's unprojection, and GetPoseInverse() of key frame 2 (read for its camera centre alone here) is given that very point as its centre
    p = one_match(X, near, True, False)
    c = R.camera(K5, SCALE)
    Xf = R.unproject_stereo(c, [[f32(v) for v in row] for row in p["Twc1"]], p["kf1"]["xy"][0], f32(p["kf1"]["depth"][0]))
    p["Twc2"] = p["Twc2"].copy(); p["Twc2"][:3, 3] = Xf
    out["zero_distance"] = (p, 7, 1)
    out["scale_inconsistent"] = (one_match(X, 0.3, oct1=7, oct2=0), 8, 0)      # ratioOctave = 1.2^7 = 3.58 against ratioDist 0.99 and ratioFactor 1.8
    out["scale_consistent_octaves"] = (one_match(X, 0.3, oct1=3, oct2=1), 0, 0)
    return out


def line_desc(k):
    """32-byte descriptor with the first k bits set: hamming(line_desc(a), line_desc(b)) = |a - b|"""
    return np.packbits(np.arange(256) < k)


def mp_item(points, n_kf, rng=None, flags=(True, True), sentinel=True):
    """points: list of dict(x3Dw, obs = [(key frame, bad, octave, desc)], ref) -> the dict ORBmatcher.UpdateMapPoints takes; with sentinel the map's values are
    0xAB / 7.0, so that what the call leaves untouched shows"""
    rng = rng or np.random.RandomState(0)
    n = len(points)
    obs = [o for p in points for o in p["obs"]]
    it = dict(Ow=rng.uniform(-3, 3, (n_kf, 3)).astype(f32), x3Dw=np.array([p["x3Dw"] for p in points], f32).reshape(n, 3),
              obs_start=np.cumsum([0] + [len(p["obs"]) for p in points]).astype(np.int32), obs_kf=np.array([o[0] for o in obs], np.int32), obs_bad=np.array([o[1] for o in obs], np.uint8),
              obs_octave=np.array([o[2] for o in obs], np.int32), obs_desc=np.array([o[3] for o in obs], np.uint8).reshape(len(obs), 32), ref_obs=np.array([p["ref"] for p in points], np.int32),
              do_descriptor=flags[0], do_normal=flags[1])
    if sentinel:
        it.update(desc=np.full((n, 32), 0xAB, np.uint8), normal=np.full((n, 3), 7.0, f32), max_dist=np.full(n, 7.0, f32), min_dist=np.full(n, 7.0, f32))
    return it


def mp_scene(seed, counts, bad=0.15, flags=(True, True), n_kf=None):
    """points with the given numbers of observations each: a random descriptor per point with up to 12 flipped bits per observation (so medians tie), key frames bad with
    probability `bad`, random octaves and reference positions"""
    rng = np.random.RandomState(seed)
    n_kf = n_kf or max(max(counts, default=0), 4) + 3
    kf_bad = rng.rand(n_kf) < bad
    pts = []
    for c in counts:
        base = rng.randint(0, 256, 32).astype(np.uint8); ks = np.sort(rng.choice(n_kf, c, replace=False))
        obs = []
        for k in ks:
            d = base.copy()
            for bit in rng.randint(0, 256, rng.randint(0, 13)): d[bit >> 3] ^= np.uint8(1 << (bit & 7))
            obs.append((int(k), int(kf_bad[k]), int(rng.randint(0, len(SCALE))), d))
        pts.append(dict(x3Dw=rng.uniform(-2, 2, 3) + np.array([0, 0, 6.0]), obs=obs, ref=int(rng.randint(c)) if c else -1))
    return mp_item(pts, n_kf, rng, flags)


def mp_literal_cases():
    """-> {name: (item, expected best_obs per point or None)}"""
    L = line_desc; P = lambda obs, ref=0: dict(x3Dw=[0.3, -0.2, 5.0], obs=obs, ref=ref)
    o = lambda k, d, bad=0, octave=0: (k, bad, octave, L(d))
    out = {}
    out["N=1"] = (mp_item([P([o(0, 17)])], 4), [0])
    out["N=2"] = (mp_item([P([o(0, 17), o(2, 90)])], 4), [0])                                    # both medians are the zero to itself: the first row
    out["N=3_tie_first_wins"] = (mp_item([P([o(0, 0), o(1, 10), o(3, 15)])], 4), [1])           # medians 10, 5, 5
    out["identical"] = (mp_item([P([o(0, 40), o(1, 40), o(2, 40), o(3, 40)])], 4), [0])
    out["all_bad"] = (mp_item([P([o(0, 17, 1), o(2, 90, 1)], ref=1)], 4), [-1])
    out["no_observations"] = (mp_item([dict(x3Dw=[0.3, -0.2, 5.0], obs=[], ref=-1)], 4), [-1])
    out["bad_would_have_won"] = (mp_item([P([o(0, 0), o(1, 50, 1), o(2, 100), o(3, 130)])], 4), [2])      # with it: medians 50, 50, 50, 80 -> 0; without: 100, 30, 30 -> position 2
    out["N=4_even"] = (mp_item([P([o(0, 0), o(1, 1), o(2, 11), o(3, 12)])], 4), [0])            # index (int)1.5 = 1: every median is 1; index 2 would give position 1
    out["N=5_odd"] = (mp_item([P([o(0, 0), o(1, 1), o(2, 2), o(3, 20), o(4, 21)])], 5), [1])    # index 2: medians 2, 1, 2, 18, 19; index 1 -> 0, index 3 -> 2
    # the normal: a bad key frame counts in n; the reference key frame first, in the middle, last; octave 0 and nlevels - 1
    top = len(SCALE) - 1
    out["normal_cases"] = (mp_item([P([o(0, 5), o(1, 9, 1), o(2, 30)], ref=0), P([o(0, 5, 0, top), o(1, 9, 0, top), o(2, 30, 0, top)], ref=1),
                                    P([o(1, 5), o(2, 9), o(3, 30, 0, top)], ref=2), P([o(3, 77, 1, top)], ref=0)], 4), [0, 0, 0, -1])       # medians 4, 4, 21: the first
    return out


def mp_bad_items():
    """items that must be refused with SIND_E_ARG -> {name: item}"""
    b = mp_scene(31, [3, 1, 5, 2])
    cp = lambda: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    out = {}
    a = cp(); a["obs_start"][0] = 1; out["obs_start does not start at 0"] = a
    a = cp(); a["obs_start"][2] = a["obs_start"][1] - 1; out["obs_start decreases"] = a
    a = cp(); a["obs_kf"][3] = len(a["Ow"]); out["obs_kf too large"] = a
    a = cp(); a["obs_kf"][3] = -1; out["obs_kf negative"] = a
    a = cp(); a["obs_octave"][2] = len(SCALE); out["octave too large"] = a
    a = cp(); a["obs_octave"][2] = -1; out["octave negative"] = a
    a = cp(); a["ref_obs"][0] = 3; out["ref_obs beyond the list"] = a
    a = cp(); a["ref_obs"][2] = -2; out["ref_obs below -1"] = a
    a = cp(); a["ref_obs"][2] = -1; out["ref_obs -1 with observations and do_normal"] = a
    a = cp(); a["x3Dw"][1, 2] = np.nan; out["position not finite"] = a
    a = cp(); a["Ow"][0, 0] = np.inf; out["camera centre not finite"] = a
    return out


def tri_bad_pairs():
    """pairs that must be refused with SIND_E_ARG -> {name: pair}"""
    b = tri_scene(41, 12, "mixed")
    def cp():
        return {k: ({q: w.copy() for q, w in v.items()} if isinstance(v, dict) else v.copy()) for k, v in b.items()}
    i = int(np.nonzero(b["match12"] >= 0)[0][0])
    out = {}
    a = cp(); a["match12"][i] = len(a["kf2"]["octave"]); out["match12 too large"] = a
    a = cp(); a["match12"][i] = -2; out["match12 below -1"] = a
    a = cp(); a["kf1"]["octave"][3] = len(SCALE); out["octave1 too large"] = a
    a = cp(); a["kf2"]["octave"][3] = -1; out["octave2 negative"] = a
    a = cp(); a["Tcw2"][1, 3] = np.nan; out["pose not finite"] = a
    a = cp(); a["Twc1"][0, 0] = np.inf; out["inverse pose not finite"] = a
    a = cp(); a["kf1"]["u_right"][i] = 100.0; a["kf1"]["depth"][i] = 0.0; out["stereo without depth"] = a
    return out


def toy_map(seed, n_kf=5, n_pts=260, mapped=0.4, share=0.9):
    """A map of plain dicts for sindslam_amd.mapping: n_kf key frames on an arc 0.6 m apart (ids 0 .. n_kf - 1) and one more 0.03 m from the middle one (closer than mb:
    the baseline test drops it); each sees a share of the points in its own slot order, a third of the slots monocular; a point's observations share a vocabulary node,
    a pyramid level, an angle and a descriptor up to 3 bits.  A share `mapped` of the points are map points already (observed wherever seen), the others wait for CreateNewMapPoints: the
    current key frame meets each of them again with every neighbour.  -> keyframes, mappoints, the id of the current key frame"""
    rng = np.random.RandomState(seed)
    ang = list(np.linspace(-0.2, 0.2, n_kf)); cur = n_kf // 2; ang.append(ang[cur] + 0.005)
    X = np.stack([rng.uniform(-2.0, 2.0, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4.5, 7.5, n_pts)], 1)
    base = rng.randint(0, 256, (n_pts, 32)).astype(np.uint8); node = (100 + np.arange(n_pts) % 37).astype(np.int32); pang = rng.uniform(0, 360, n_pts)
    poct = rng.randint(0, 3, n_pts)                                     # a point keeps its pyramid level from key frame to key frame (they are equally far away)
    is_mp = rng.rand(n_pts) < mapped
    ids = {int(p): i for i, p in enumerate(np.nonzero(is_mp)[0])}
    mappoints = {i: dict(x3Dw=(X[p] + rng.normal(0, 0.01, 3)).astype(f32), obs={}, bad=False) for p, i in ids.items()}
    keyframes = {}
    for k, a in enumerate(ang):
        T = LS.arc_pose(a).astype(f32)
        see = rng.permutation(np.nonzero(rng.rand(n_pts) < share)[0]); n = len(see)
        un = np.zeros((n, 2), f32); ur = np.full(n, -1, f32); dp = np.full(n, -1, f32); desc = np.zeros((n, 32), np.uint8); mp = np.full(n, -1, np.int64)
        for sl, p in enumerate(see):
            u, v, r, z = LS.project(T.astype(np.float64), X[p], K5); e = rng.normal(0, 0.3, 3)
            un[sl] = (u + e[0], v + e[1])
            if (sl + k) % 3:
                ur[sl] = r + e[2]; dp[sl] = z
            d = base[p].copy()
            for bit in rng.randint(0, 256, rng.randint(0, 4)): d[bit >> 3] ^= np.uint8(1 << (bit & 7))
            desc[sl] = d
            if int(p) in ids:
                mp[sl] = ids[int(p)]; mappoints[ids[int(p)]]["obs"][k] = sl
        keyframes[k] = dict(Tcw=T, un_xy=un, xy=un + f32(0.25), octave=poct[see].astype(np.int32), u_right=ur, depth=dp, desc=desc, node=node[see], angle=((pang[see] + rng.uniform(-3, 3, n)) % 360).astype(f32),
                            mp=mp, bad=False, inv_sigma2=np.ones(n, f32), point_of_slot=see)
        keyframes[k]["inv_sigma2"] = (1.0 / (SCALE[keyframes[k]["octave"]] ** 2)).astype(f32)
    for m, p in mappoints.items():
        p["ref_kf"] = min(p["obs"]) if p["obs"] else 0
    for k in keyframes:
        w = {q: len(set(keyframes[k]["mp"][keyframes[k]["mp"] >= 0].tolist()) & set(keyframes[q]["mp"][keyframes[q]["mp"] >= 0].tolist())) for q in keyframes if q != k}
        keyframes[k]["covisible"] = sorted(w, key=lambda q: (-w[q], q))
    return keyframes, mappoints, cur


def literal_create_new_map_points(matcher, kf_id, keyframes, mappoints, nn=10):
    """CreateNewMapPoints as the reference runs it: neighbour after neighbour, every search on the key frame as the earlier neighbours left it, every new point updated at
    once.  -> the ids of the new points"""
    from sindslam_amd import mapping as M
    cur = keyframes[kf_id]; new = []
    for k in M.neighbours_for_triangulation(matcher, kf_id, keyframes, nn):
        kf2 = keyframes[k]
        m12 = matcher.SearchForTriangulation([(np.asarray(kf2["Tcw"], f32), M.camera_centre(cur), M.compute_f12(cur, kf2, matcher.K5), M._search_side(cur), M._search_side(kf2))], False)[0][0]
        r = matcher.Triangulate([dict(Tcw1=cur["Tcw"], Twc1=M.pose_inverse(cur), Tcw2=kf2["Tcw"], Twc2=M.pose_inverse(kf2), kf1=M._tri_side(cur), kf2=M._tri_side(kf2), match12=m12)])[0]
        for idx1 in np.nonzero(m12 >= 0)[0].tolist():
            if r["status"][idx1] != 0:
                continue
            m = M._add_new_point(kf_id, k, idx1, m12[idx1], r["x3D"][idx1], keyframes, mappoints)
            M.update_map_points(matcher, [m], keyframes, mappoints)
            new.append(m)
    return new


def same_maps(a, b):
    """two maps (keyframes, mappoints) equal: ids, slots, observation sets, and the point values as bit patterns"""
    (ka, ma), (kb, mb) = a, b
    assert sorted(ma) == sorted(mb) and sorted(ka) == sorted(kb)
    for k in ka:
        assert np.array_equal(ka[k]["mp"], kb[k]["mp"]), k
        assert np.asarray(ka[k]["Tcw"], f32).tobytes() == np.asarray(kb[k]["Tcw"], f32).tobytes(), k
    for m in ma:
        assert ma[m]["obs"] == mb[m]["obs"] and bool(ma[m].get("bad")) == bool(mb[m].get("bad")), m
        for key in ("x3Dw", "normal", "max_dist", "min_dist", "desc"):
            assert (ma[m].get(key) is None) == (mb[m].get(key) is None), (m, key)
            if ma[m].get(key) is not None:
                assert np.asarray(ma[m][key]).tobytes() == np.asarray(mb[m][key]).tobytes(), (m, key)


def build_grid(un_xy, bounds=(0.0, 640.0, 0.0, 480.0)):
    """mGrid of a key frame as grid_start [3073] / grid_idx (cell = ix * 48 + iy, push_back order inside a cell), from Frame::PosInGrid's rounding"""
    un = np.asarray(un_xy, f32)
    wi = f32(64) / f32(bounds[1] - bounds[0]); hi = f32(48) / f32(bounds[3] - bounds[2])
    rnd = lambda v: (np.sign(v) * np.floor(np.abs(v) + f32(0.5))).astype(np.int64)
    px = rnd((un[:, 0] - f32(bounds[0])) * wi); py = rnd((un[:, 1] - f32(bounds[2])) * hi)
    ok = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    cell = np.where(ok, px * 48 + py, -1)
    idx = np.nonzero(ok)[0]; idx = idx[np.argsort(cell[idx], kind="stable")]
    start = np.zeros(64 * 48 + 1, np.int32); np.add.at(start, cell[idx] + 1, 1)
    return np.cumsum(start).astype(np.int32), idx.astype(np.int32)


def local_mapping_step(mt, keyframes, mappoints, cur):
    """the local mapper's Run body on the dicts through sindslam_amd: the points of the map get their descriptors and normals, CreateNewMapPoints, Fuse of the current key
    frame's points into the neighbours with its graph tail and update_after_fuse, LocalBundleAdjustment with apply_local_ba and update_after_local_ba.  The map IS modified.
    -> (new point ids, fused count, the local BA's result)"""
    from sindslam_amd import mapping as M
    from sindslam_amd import optimizer as O
    M.update_map_points(mt, sorted(mappoints), keyframes, mappoints)
    new = M.create_new_map_points(mt, cur, keyframes, mappoints)
    nfused = 0
    for t in M.neighbours_for_triangulation(mt, cur, keyframes):
        kf = keyframes[t]
        ids = [int(m) for m in dict.fromkeys(keyframes[cur]["mp"].tolist()) if m >= 0]
        mp = dict(x3Dw=np.array([mappoints[m]["x3Dw"] for m in ids], f32), normal=np.array([mappoints[m]["normal"] for m in ids], f32), max_dist=np.array([mappoints[m]["max_dist"] for m in ids], f32),
                  min_dist=np.array([mappoints[m]["min_dist"] for m in ids], f32), valid=np.array([not mappoints[m].get("bad") and t not in mappoints[m]["obs"] for m in ids], np.uint8),
                  desc=np.array([mappoints[m]["desc"] for m in ids], np.uint8))
        gs, gi = build_grid(kf["un_xy"])
        r = mt.Fuse([(kf["Tcw"], mp, dict(un_xy=kf["un_xy"], octave=kf["octave"], u_right=kf["u_right"], desc=kf["desc"], grid_start=gs, grid_idx=gi))])[0]
        for i, idx in enumerate(r["best_idx"].tolist()):                 # Fuse's graph tail (ORBmatcher.cc:925-945)
            pid = ids[i]
            if idx < 0 or mappoints[pid].get("bad"):
                continue
            other = int(kf["mp"][idx])
            if other >= 0:
                if not mappoints[other].get("bad"):
                    if len(mappoints[other]["obs"]) > len(mappoints[pid]["obs"]): O._replace(keyframes, mappoints, pid, other)
                    else: O._replace(keyframes, mappoints, other, pid)
            else:
                mappoints[pid]["obs"][t] = idx; kf["mp"][idx] = pid
            nfused += 1
    M.update_after_fuse(mt, cur, keyframes, mappoints)
    res = O.LocalBundleAdjustment(mt, cur, keyframes, mappoints)
    O.apply_local_ba(keyframes, mappoints, res)
    O.update_after_local_ba(mt, keyframes, mappoints, res)
    return new, nfused, res
