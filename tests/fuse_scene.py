"""Test scenes for the projections of map points into a key frame (Fuse, SearchByProjection(pKF, Scw), SearchBySim3), built on localmap_scene / match_scene.
A list of map points is a dict: x3Dw, normal, max_dist, min_dist, valid, desc; a key frame: un_xy, octave, u_right, desc, grid_start, grid_idx (and taken)."""
import numpy as np

import fuse_ref as F
import localmap_ref as R
import localmap_scene as L
import match_scene as S

f32 = np.float32


def _points(mp):
    out = {k: mp[k] for k in ("x3Dw", "normal", "max_dist", "min_dist", "desc")}
    out["valid"] = (mp["flags"] & 1).astype(np.uint8)
    return out


def similarity(T, s):
    """Scw = [s Rcw | s tcw]: the pose seen from a map whose scale is off by s; its decomposition gives Rcw and tcw back up to rounding"""
    Sm = np.array(T, np.float32); Sm[:3] = (Sm[:3].astype(np.float64) * s).astype(np.float32)
    return Sm


def stream_key_frame(stream, t, seed=0, mono=0.2, taken=0.1):
    """(cam10, scale, Tcw, mp, kf): frame t-1 of the stream as the key frame against the map points of frames t-2 .. t-5; a share `mono` of its keypoints gets
    u_right = -1 (on top of those without depth), a share `taken` is in vpMatched on entry"""
    rng = np.random.default_rng(3000 + seed)
    cam, sc, Tc, mp, cur = L.stream_local_map(stream, t - 1, seed=seed)
    kf = dict(cur); n = len(kf["octave"])
    kf["u_right"] = np.where(rng.random(n) < mono, f32(-1), cur["u_right"]).astype(np.float32)
    kf["taken"] = (rng.random(n) < taken).astype(np.uint8)
    return cam, sc, Tc, _points(mp), kf


def stress_key_frame(seed):
    """the few-codes construction: many equal distances, heavily contended keypoints, a tenth of them taken"""
    cam, sc, Tc, mp, cur = L.stress_local_map(seed)
    return cam, sc, Tc, _points(mp), dict(cur)


def _at_max_x(cam, sc, Tc, rng, count):
    """points whose projection into the key frame is u == mnMaxX exactly (out for KeyFrame::IsInImage) while Frame::isInFrustum keeps them (u <= mnMaxX)"""
    fx, fy, cx, cy = [float(v) for v in cam[:4]]; max_x = f32(cam[7])
    Rcw, tcw = Tc[:3, :3].astype(np.float64), Tc[:3, 3].astype(np.float64); Ow = R.camera_centre(Tc)
    out = []
    while len(out) < count:
        v, z = rng.uniform(60, 420), rng.uniform(1.2, 3.0)
        P = (Rcw.T @ (np.array([(float(max_x) - cx) * z / fx, (v - cy) * z / fy, z]) - tcw)).astype(np.float32)
        for _ in range(400):                                                # walk x3Dw[0] by ulps until the FP32 projection is the bound itself
            PO, dist = R.distance(P, Ow)
            nrm = (np.array(PO, np.float64) / np.float64(dist)).astype(np.float32)
            mx = f32(f32(1.7) * dist); mn = f32(mx / sc[len(sc) - 1])
            Pc = R.to_camera(Tc, P); invz = f32(f32(1.0) / Pc[2]); u = f32(f32(f32(cam[0]) * f32(Pc[0] * invz)) + f32(cam[2]))
            if u == max_x: break
            P[0] = np.nextafter(P[0], f32(np.inf) if u < max_x else f32(-np.inf))
        one = dict(x3Dw=P[None], normal=nrm[None], max_dist=np.array([mx]), min_dist=np.array([mn]), flags=np.array([3], np.uint8))
        if u == max_x and R.frustum(cam, sc, Tc, one)["in_view"][0] and F.project(F.FUSE, cam, sc, Tc, Ow, P, nrm, mx, mn)[0] == R.OUT_X:
            out.append((P.copy(), nrm, mx, mn))
    return out


def branch_scene(seed=7, per_class=8):
    """localmap_scene.branch_scene's points (every exit of the projection: behind, the four image sides, too near / too far, oblique, not valid, level clamped at 0 and at
    the top, created-at-this-distance for every octave) plus the class "at_max_x".  -> (cam10, scale, Tcw, mp, kf, expect): expect[i] = (why, level or None, name)"""
    cam, sc, Tc, mp, cur, expect = L.branch_scene(seed, per_class)
    rng = np.random.default_rng(seed + 100)
    extra = _at_max_x(cam, sc, Tc, rng, per_class)
    n0 = len(mp["flags"])
    pts = _points(mp)
    pts["x3Dw"] = np.concatenate([pts["x3Dw"], np.array([e[0] for e in extra], np.float32)]); pts["normal"] = np.concatenate([pts["normal"], np.array([e[1] for e in extra], np.float32)])
    pts["max_dist"] = np.concatenate([pts["max_dist"], np.array([e[2] for e in extra], np.float32)]); pts["min_dist"] = np.concatenate([pts["min_dist"], np.array([e[3] for e in extra], np.float32)])
    pts["valid"] = np.concatenate([pts["valid"], np.ones(len(extra), np.uint8)])
    _, _, _, _, last, _ = S.stress_pair(seed)
    pts["desc"] = last["desc"][:n0 + len(extra)].copy()
    expect = [(why, lvl, name) for why, _, lvl, name in expect] + [(R.OUT_X, None, "at_max_x")] * len(extra)
    return cam, sc, Tc, pts, dict(cur), expect


_SLOTS = {}


def _slots(stream, f):
    """frame f of the stream as a key frame whose slot i holds the back-projected keypoint i as its map point -> (cam10, Tcw, side with has_point for valid); kept per frame"""
    if f not in _SLOTS:
        _SLOTS[f] = _make_slots(stream, f)
    cam, Tf, side = _SLOTS[f]
    return cam.copy(), Tf.copy(), {k: v.copy() for k, v in side.items()}


def _make_slots(stream, f):
    sc = S._scale_factors()
    cam, _, Tf, _, _, keys = S.stream_pair(stream, f, seed=f)                # cur = frame f: keypoints and grid
    _, _, _, Tl, pts, _ = S.stream_pair(stream, f + 1, seed=f)              # last = frame f: its keypoints back-projected
    assert len(pts["octave"]) == len(keys["octave"]) and np.array_equal(pts["desc"], keys["desc"]) and np.array_equal(Tl, Tf)
    d = np.linalg.norm(pts["x3Dw"].astype(np.float64) - R.camera_centre(Tf).astype(np.float64), axis=1)
    mx, mn = L._invariance(d, pts["octave"], sc)
    return cam, Tf, dict(has_point=pts["valid"] > 0, x3Dw=pts["x3Dw"], max_dist=mx, min_dist=mn, mp_desc=pts["desc"], un_xy=keys["un_xy"], octave=keys["octave"], kf_desc=keys["desc"],
                    grid_start=keys["grid_start"], grid_idx=keys["grid_idx"])


def sim3_pair(stream, t, seed=0, scale=1.08, matched=0.15):
    """(cam10, scale factors, T1w, T2w, s12, R12, t12, side1, side2): frames t-1 and t as key frames with their own map points, pKF2 and its points living in a map
    scaled by `scale` (so s12 = 1 / scale), the true relative similarity given; a share `matched` of the slots is pre-matched (vbAlreadyMatched1/2)"""
    rng = np.random.default_rng(4000 + seed)
    sc = S._scale_factors()
    cam, T1, s1 = _slots(stream, t - 1); _, T2, s2 = _slots(stream, t)
    a = float(scale)
    T2s = T2.copy(); T2s[:3, 3] = (T2[:3, 3].astype(np.float64) * a).astype(np.float32)
    s2["x3Dw"] = (s2["x3Dw"].astype(np.float64) * a).astype(np.float32); s2["max_dist"] = (s2["max_dist"] * f32(a)).astype(np.float32); s2["min_dist"] = (s2["min_dist"] * f32(a)).astype(np.float32)
    R1, t1, R2, t2 = T1[:3, :3].astype(np.float64), T1[:3, 3].astype(np.float64), T2[:3, :3].astype(np.float64), T2[:3, 3].astype(np.float64)
    R12 = R1 @ R2.T; t12 = t1 - R12 @ t2                                     # p_c1 = R12 p_c2 + t12 in the unscaled map; p_c2' = a p_c2
    for s in (s1, s2):
        s["valid"] = (s.pop("has_point") & (rng.random(len(s["octave"])) > matched)).astype(np.uint8)
    return cam, sc, T1, T2s, f32(1.0 / a), R12.astype(np.float32), t12.astype(np.float32), s1, s2


def branch_sim3_pair(stream, seed=7):
    """sim3_pair(stream, 6) with the points of branch_scene in the first slots of side 1, re-expressed for pKF1's pose: the exits of SearchBySim3 (behind, the image
    sides, too near / too far, not valid) among slots that otherwise match.  -> (cam10, ..., side2, n): n slots hold branch points"""
    cam, sc, T1, T2, s12, R12, t12, s1, s2 = sim3_pair(stream, 6, seed=6)
    _, _, Tc, mp, _, _ = branch_scene(seed)
    n = len(mp["valid"])
    pc = mp["x3Dw"].astype(np.float64) @ Tc[:3, :3].T.astype(np.float64) + Tc[:3, 3].astype(np.float64)
    s1["x3Dw"][:n] = ((pc - T1[:3, 3].astype(np.float64)) @ T1[:3, :3].astype(np.float64)).astype(np.float32)
    s1["max_dist"][:n] = mp["max_dist"]; s1["min_dist"][:n] = mp["min_dist"]; s1["valid"][:n] = mp["valid"]
    return cam, sc, T1, T2, s12, R12, t12, s1, s2, n


def stress_sim3_pair(stream, seed, n_codes=6):
    """sim3_pair(stream, 6) with the few-codes construction on both sides: a slot's map point and its keypoint share one of n_codes descriptors (2 % of the bytes flipped),
    so windows hold many equal distances and slots contend for keypoints"""
    rng = np.random.default_rng(6000 + seed)
    cam, sc, T1, T2, s12, R12, t12, s1, s2 = sim3_pair(stream, 6, seed=seed, scale=0.93)
    codes = rng.integers(0, 256, (n_codes, 32)).astype(np.uint8)
    flip = lambda d: d ^ (rng.random(d.shape) < 0.02).astype(np.uint8) * rng.integers(1, 255, d.shape).astype(np.uint8)
    for s in (s1, s2):
        c = codes[rng.integers(0, n_codes, len(s["valid"]))]
        s["mp_desc"] = flip(c); s["kf_desc"] = flip(c)
    return cam, sc, T1, T2, s12, R12, t12, s1, s2


def toy_graph(seed, n_list=400, resident=0.5):
    """A Graph over the stress scene's key frame, as key frame 0 (and 1, the same keypoints, for the batching counter-case).  The list: n_list map points, each a
    keypoint of the key frame back-projected at its depth (2 m) with up to 0.7 px of jitter and that keypoint's descriptor, one to four points per keypoint, with one to
    four observations in other key frames, 5 % bad.  A share `resident` of the keypoints the snapshot search hits already holds a resident point (a third of the
    residents bad, the others with zero to five observations besides); the list repeats a tenth of its entries, holds NULLs and is shuffled.
    -> (graph, cam10, scale, Tcw, kf, plist)"""
    rng = np.random.default_rng(5000 + seed)
    cam, sc, Tc, _, kf = stress_key_frame(seed)
    fx, fy, cx, cy = [float(v) for v in cam[:4]]
    Rcw, tcw = Tc[:3, :3].astype(np.float64), Tc[:3, 3].astype(np.float64); Ow = R.camera_centre(Tc)
    g = F.Graph()
    while len(g.points) < n_list:
        k = int(rng.integers(0, len(kf["octave"])))
        for _ in range(int(rng.integers(1, 5))):
            u, v = kf["un_xy"][k] + rng.uniform(-0.7, 0.7, 2)
            P = (Rcw.T @ (np.array([(u - cx) * 2.0 / fx, (v - cy) * 2.0 / fy, 2.0]) - tcw)).astype(np.float32)
            PO, dist = R.distance(P, Ow)
            mx = f32(dist * sc[kf["octave"][k]])
            pid = g.add_point(P, np.array(PO, np.float64) / np.float64(dist), mx, f32(mx / sc[len(sc) - 1]), kf["desc"][k], bad=rng.random() < 0.05)
            for j in range(int(rng.integers(1, 5))): g.observe(pid, 100 + j, 10 * pid + j)
    n_list = len(g.points); plist = list(range(n_list))
    hit = F.fuse_search(cam, sc, Tc, g.inputs(0, plist, False), kf, 3.0, False)["best_idx"]
    for idx in sorted(set(int(b) for b in hit if b >= 0)):
        if rng.random() < resident:
            pid = g.add_point((0, 0, 1), (0, 0, 1), 1, 1, rng.integers(0, 256, 32), bad=rng.random() < 0.33)
            for kf_id in (0, 1): g.observe(pid, kf_id, idx)
            for j in range(int(rng.integers(0, 6))): g.observe(pid, 200 + j, 10 * pid + j)
    plist += [int(p) for p in rng.integers(0, n_list, n_list // 10)] + [-1] * 5
    order = rng.permutation(len(plist))
    return g, cam, sc, Tc, kf, [plist[j] for j in order], n_list
