"""Test scenes for the map-point projection searches (local map, relocalisation), built on match_scene (ORACLE extractor / Frame steps).
A set of map points is a dict: x3Dw, normal, max_dist, min_dist, flags (bit0 candidate, bit1 observed), desc."""
import numpy as np

import localmap_ref as R
import match_scene as S

f32 = np.float32


def _tilt(normals, deg, rng):
    """unit vectors turned by deg (per row) about a random axis perpendicular to them"""
    n = normals.astype(np.float64); a = np.cross(n, rng.normal(size=n.shape)); a /= np.linalg.norm(a, axis=1)[:, None]
    th = np.deg2rad(deg)[:, None]
    return (n * np.cos(th) + a * np.sin(th)).astype(np.float32)


def _invariance(dist, octave, sc):
    """mfMaxDistance, mfMinDistance as MapPoint.cc:63-64 computes them from the observing distance and octave (FP32)"""
    mx = (dist.astype(np.float32) * sc[octave]).astype(np.float32)
    return mx, (mx / sc[len(sc) - 1]).astype(np.float32)


def _observed(Tl, last):
    """the valid keypoints of a frame as map points seen from that frame: positions, unit viewing directions, distances"""
    ok = last["valid"] > 0
    Ow = R.camera_centre(Tl).astype(np.float64)
    P = last["x3Dw"][ok]; PO = P.astype(np.float64) - Ow; d = np.linalg.norm(PO, axis=1)
    return ok, P, (PO / d[:, None]).astype(np.float32), d


def stream_local_map(stream, t, seed=0, depth=4):
    """(cam10, scale, Tcw, mp, cur): frame t of the synthetic stream at its ground-truth pose against the back-projected keypoints of frames
    t-1 .. t-depth (duplicates of the same surface point -> contended keypoints).  85 % of the normals are the exact viewing directions, 10 %
    are tilted by 2-8 degrees (viewCos on both sides of 0.998), 5 % by 65-85 degrees (the viewing-angle exit)."""
    rng = np.random.default_rng(1000 + seed); sc = S._scale_factors()
    xs, ns, mx, mn, ds = [], [], [], [], []
    for k in range(1, depth + 1):
        _, _, _, Tl, last, _ = S.stream_pair(stream, t - k + 1, seed=seed + k)          # last = frame t-k
        ok, P, nrm, d = _observed(Tl, last)
        a, b = _invariance(d, last["octave"][ok], sc)
        xs.append(P); ns.append(nrm); mx.append(a); mn.append(b); ds.append(last["desc"][ok])
    cam, _, Tc, _, _, cur = S.stream_pair(stream, t, seed=seed)
    n = sum(len(x) for x in xs)
    cls = rng.random(n); deg = np.where(cls < 0.85, 0.0, np.where(cls < 0.95, rng.uniform(2, 8, n), rng.uniform(65, 85, n)))
    mp = dict(x3Dw=np.concatenate(xs), normal=_tilt(np.concatenate(ns), deg, rng), max_dist=np.concatenate(mx), min_dist=np.concatenate(mn), desc=np.concatenate(ds),
              flags=((rng.random(n) > 0.05) * 1 + (rng.random(n) < 0.9) * 2).astype(np.uint8))
    return cam, sc, Tc, mp, cur


def stress_local_map(seed):
    """stress_pair's few-codes construction as a local map: many equal distances, a tenth of the keypoints taken, 60 % of the points observed"""
    cam, sc, Tc, Tl, last, cur = S.stress_pair(seed)
    P = last["x3Dw"]; d = np.linalg.norm(P.astype(np.float64), axis=1)                   # created from the identity pose Tl
    mx, mn = _invariance(d, last["octave"], sc)
    mp = dict(x3Dw=P, normal=(P / d[:, None]).astype(np.float32), max_dist=mx, min_dist=mn, desc=last["desc"], flags=(last["valid"] * 1 + last["has_obs"] * 2).astype(np.uint8))
    return cam, sc, Tc, mp, cur


def branch_scene(seed=7, per_class=8):
    """Synthetic points built to take every exit of Frame::isInFrustum, both radius classes, level clamping at both ends, and dist == creation
    distance for every octave.  -> (cam10, scale, Tcw, mp, cur, expect): expect[i] = (why, radius class or None, level or None, name)."""
    rng = np.random.default_rng(seed)
    cam, sc, Tc, _, last, cur = S.stress_pair(seed)
    fx, fy, cx, cy = [float(v) for v in cam[:4]]
    Rcw, tcw = Tc[:3, :3].astype(np.float64), Tc[:3, 3].astype(np.float64)
    Ow = R.camera_centre(Tc)
    top = len(sc) - 1
    # name, u range, v range, z sign, max_dist / dist (None: dist * scale[octave]), tilt of the normal in degrees, expected exit; min_dist = max_dist / scale[top]
    inside = ((60, 580), (60, 420))
    classes = [("behind", *inside, -1, 1.0, 0, R.BEHIND), ("left", (-80, -20), (60, 420), 1, 1.0, 0, R.OUT_X), ("right", (660, 720), (60, 420), 1, 1.0, 0, R.OUT_X),
               ("above", (60, 580), (-80, -20), 1, 1.0, 0, R.OUT_Y), ("below", (60, 580), (500, 560), 1, 1.0, 0, R.OUT_Y),
               ("too_near", *inside, 1, 10.0, 0, R.OUT_DIST), ("too_far", *inside, 1, 1 / 1.5, 0, R.OUT_DIST), ("oblique", *inside, 1, 1.0, 70, R.OUT_ANGLE),
               ("not_candidate", *inside, 1, 1.0, 0, R.NOT_CANDIDATE),
               ("narrow", *inside, 1, 1.7, 0, R.IN_VIEW), ("wide", *inside, 1, 1.7, 10, R.IN_VIEW),
               ("level_0", *inside, 1, 0.85, 0, R.IN_VIEW), ("level_top", *inside, 1, 4.2, 0, R.IN_VIEW)]
    classes += [(f"created_{o}", *inside, 1, None, 0, R.IN_VIEW) for o in range(len(sc))]
    X, N, MX, MN, FL, expect = [], [], [], [], [], []
    for name, ur, vr, zs, ratio, tilt, why in classes:
        for _ in range(per_class):
            while True:
                u, v, z = rng.uniform(*ur), rng.uniform(*vr), zs * rng.uniform(1.2, 3.0)
                pc = np.array([(u - cx) * z / fx, (v - cy) * z / fy, z])
                P = (Rcw.T @ (pc - tcw)).astype(np.float32)
                PO, dist = R.distance(P, Ow)
                if ratio is not None:
                    mx = f32(f32(ratio) * dist); break
                o = int(name.split("_")[1]); mx = f32(dist * sc[o])                         # seen again at the distance it was created at
                if f32(mx / dist) == sc[o]: break                                           # keep the draws whose FP32 quotient is scale[o] exactly
            nrm = (np.array(PO, np.float64) / np.float64(dist)).astype(np.float32)[None]
            X.append(P); N.append(_tilt(nrm, np.array([float(tilt)]), rng)[0]); MX.append(mx); MN.append(f32(mx / sc[top])); FL.append(2 if name == "not_candidate" else 3)
            rc = None if why != R.IN_VIEW else ("wide" if name == "wide" else "narrow")
            lvl = {"level_0": 0, "level_top": top}.get(name, int(name.split("_")[1]) if ratio is None else None)
            expect.append((why, rc, lvl, name))
    n = len(X)
    mp = dict(x3Dw=np.array(X, np.float32), normal=np.array(N, np.float32), max_dist=np.array(MX, np.float32), min_dist=np.array(MN, np.float32), flags=np.array(FL, np.uint8),
              desc=last["desc"][:n].copy())
    return cam, sc, Tc, mp, cur, expect


def reloc_pair(stream, t, seed=0, found=0.15, held=0.05):
    """(cam10, scale, Tcw_cur, kf, cur): frame t-1 of the stream as the key frame (its keypoints are the slots), frame t as the current frame at its
    ground-truth pose; a share `found` of the slots is in sAlreadyFound, a share `held` of the current keypoints already holds a map point."""
    rng = np.random.default_rng(2000 + seed); sc = S._scale_factors()
    cam, _, Tc, Tl, last, cur = S.stream_pair(stream, t, seed=seed)
    Ow = R.camera_centre(Tl).astype(np.float64)
    d = np.linalg.norm(last["x3Dw"].astype(np.float64) - Ow, axis=1)
    mx, mn = _invariance(d, last["octave"], sc)
    kf = dict(x3Dw=last["x3Dw"], max_dist=mx, min_dist=mn, valid=((last["valid"] > 0) & (rng.random(len(d)) > found)).astype(np.uint8), angle=last["angle"], desc=last["desc"])
    cur = dict(cur); cur["taken"] = (rng.random(len(cur["octave"])) < held).astype(np.uint8)
    return cam, sc, Tc, kf, cur
