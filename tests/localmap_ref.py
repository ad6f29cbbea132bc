"""Plain Python restatement of the reference's map-point projection searches (test infrastructure; nothing under sindslam_amd/ imports it):
  frustum()      Frame::isInFrustum (src/Frame.cc:340-396) + MapPoint::PredictScale (src/MapPoint.cc:402-418) over a list of map points,
  search_local() ORBmatcher::SearchByProjection(F, vpMapPoints, th) + RadiusByViewingCos (src/ORBmatcher.cc:45-137),
  search_kf()    ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1472-1599),
  features_in_area() Frame::GetFeaturesInArea (src/Frame.cc:398-451) on the CSR grid.
Sequential loops, numpy.float32 / float64 scalars placed where the reference (and the OpenCV 4.2.0 calls it makes) round; the FP32 std::log of
PredictScale and Frame::mfLogScaleFactor is DEFINED as the FP64 logarithm rounded to FP32 (see sindslam_amd/csrc/match_local.hip).
cam10 = (fx, fy, cx, cy, bf, mb, mnMinX, mnMaxX, mnMinY, mnMaxY) as match_scene builds it."""
import numpy as np

f32, f64 = np.float32, np.float64
TH_HIGH, HISTO_LENGTH = 100, 30
# why a point left isInFrustum
IN_VIEW, BEHIND, OUT_X, OUT_Y, OUT_DIST, OUT_ANGLE, NOT_CANDIDATE = 0, 1, 2, 3, 4, 5, 9


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def camera_centre(T):
    """mOw = -Rcw^T * tcw: FP64 accumulation, times -1, to FP32"""
    T = np.asarray(T, np.float32)
    return np.array([f32(sum(f64(T[k, r]) * f64(T[k, 3]) for k in range(3)) * f64(-1.0)) for r in range(3)], np.float32)


def to_camera(T, P):
    """Rcw * P + tcw: FP32 row product, then FP64 addition of tcw"""
    return [f32(f64(f32(f32(f32(T[r, 0] * P[0]) + f32(T[r, 1] * P[1])) + f32(T[r, 2] * P[2]))) + f64(T[r, 3])) for r in range(3)]


def distance(P, Ow):
    """(PO, cv::norm(PO)) for PO = P - Ow in FP32; the norm accumulates in FP64"""
    PO = [f32(P[k] - Ow[k]) for k in range(3)]
    return PO, f32(np.sqrt(sum(f64(x) * f64(x) for x in PO)))


def log_scale_factor(sc):
    return f32(np.log(f64(sc[1])))


def predict_scale(max_dist, dist, sc):
    ratio = f32(f32(max_dist) / dist)
    n = int(np.ceil(f32(f32(np.log(f64(ratio))) / log_scale_factor(sc))))
    return 0 if n < 0 else (len(sc) - 1 if n >= len(sc) else n)


def frustum(cam, sc, T, mp, limit=0.5):
    fx, fy, cx, cy, bf = [f32(v) for v in cam[:5]]; b = [f32(v) for v in cam[6:10]]; limit = f32(limit)
    T = np.asarray(T, np.float32); Ow = camera_centre(T)
    n = len(mp["flags"])
    out = dict(in_view=np.zeros(n, np.uint8), proj_xyr=np.zeros((n, 3), np.float32), level=np.zeros(n, np.int32), view_cos=np.zeros(n, np.float32),
               why=np.zeros(n, np.int32), n_to_match=0)
    for i in range(n):
        if not (mp["flags"][i] & 1):
            out["why"][i] = NOT_CANDIDATE; continue
        P = mp["x3Dw"][i]
        Pc = to_camera(T, P)
        if Pc[2] < f32(0.0):
            out["why"][i] = BEHIND; continue
        invz = f32(f32(1.0) / Pc[2])
        u = f32(f32(f32(fx * Pc[0]) * invz) + cx); v = f32(f32(f32(fy * Pc[1]) * invz) + cy)
        if u < b[0] or u > b[1]:
            out["why"][i] = OUT_X; continue
        if v < b[2] or v > b[3]:
            out["why"][i] = OUT_Y; continue
        PO, dist = distance(P, Ow)
        if dist < f32(f32(0.8) * mp["min_dist"][i]) or dist > f32(f32(1.2) * mp["max_dist"][i]):
            out["why"][i] = OUT_DIST; continue
        vc = f32(sum(f64(PO[k]) * f64(mp["normal"][i][k]) for k in range(3)) / f64(dist))
        if vc < limit:
            out["why"][i] = OUT_ANGLE; continue
        out["in_view"][i] = 1; out["proj_xyr"][i] = (u, v, f32(u - f32(bf * invz))); out["level"][i] = predict_scale(mp["max_dist"][i], dist, sc); out["view_cos"][i] = vc
        out["n_to_match"] += 1
    return out


def features_in_area(cam, cur, x, y, r, min_level, max_level):
    b = [f32(v) for v in cam[6:10]]
    w_inv = f32(f32(64) / f32(b[1] - b[0])); h_inv = f32(f32(48) / f32(b[3] - b[2]))
    x0 = max(0, int(np.floor(f32(f32(f32(x - b[0]) - r) * w_inv))))
    if x0 >= 64: return []
    x1 = min(63, int(np.ceil(f32(f32(f32(x - b[0]) + r) * w_inv))))
    if x1 < 0: return []
    y0 = max(0, int(np.floor(f32(f32(f32(y - b[2]) - r) * h_inv))))
    if y0 >= 48: return []
    y1 = min(47, int(np.ceil(f32(f32(f32(y - b[2]) + r) * h_inv))))
    if y1 < 0: return []
    gs, gi, oc, xy = cur["grid_start"], cur["grid_idx"], cur["octave"], cur["un_xy"]
    check = min_level > 0 or max_level >= 0
    out = []
    for ix in range(x0, x1 + 1):
        for j in range(gs[ix * 48 + y0], gs[ix * 48 + y1 + 1]):            # cells (ix, y0..y1) are contiguous in the CSR
            k = gi[j]
            if check and (oc[k] < min_level or (max_level >= 0 and oc[k] > max_level)): continue
            if abs(f32(xy[k, 0] - x)) < r and abs(f32(xy[k, 1] - y)) < r: out.append(int(k))
    return out


def radius_by_viewing_cos(view_cos):
    return f32(2.5) if f64(view_cos) > 0.998 else f32(4.0)


def local_radius(view_cos, th, sc, level):
    r = radius_by_viewing_cos(view_cos)
    if f32(th) != f32(1.0): r = f32(r * f32(th))
    return f32(r * sc[level])


def search_local(cam, sc, mp, cur, fr, th, nnratio=0.8, sequential=True):
    """-> match_of_cur, nmatches, choice [n_points], stats.  sequential=False searches every point against the frame as it was on entry
    (the count of choices that then differ is how much of the reference's sequential dependence a scene exercises)."""
    n_cur = len(cur["octave"]); nnratio = f32(nnratio)
    closed = np.zeros(n_cur, np.uint8) if cur.get("taken") is None else np.array(cur["taken"], np.uint8)
    closed0 = closed.copy()
    m = np.full(n_cur, -1, np.int32); nm = 0; choice = np.full(len(mp["flags"]), -1, np.int32); stats = dict(same_level=0, rejected=0)
    for i in range(len(mp["flags"])):
        if not fr["in_view"][i]: continue
        lv = int(fr["level"][i]); x, y, xr = fr["proj_xyr"][i]
        rad = local_radius(fr["view_cos"][i], th, sc, lv)
        bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
        for k in features_in_area(cam, cur, x, y, rad, lv - 1, lv):
            if (closed if sequential else closed0)[k]: continue
            if cur["u_right"][k] > 0 and abs(f32(xr - cur["u_right"][k])) > rad: continue
            d = hamming(mp["desc"][i], cur["desc"][k])
            if d < bd: bd2, bd, bl2, bl, bi = bd, d, bl, int(cur["octave"][k]), k
            elif d < bd2: bl2, bd2 = int(cur["octave"][k]), d
        if bd <= TH_HIGH:
            if bl == bl2:
                stats["same_level"] += 1
                if f32(bd) > f32(nnratio * f32(bd2)):
                    stats["rejected"] += 1; continue
            m[bi] = i; nm += 1; choice[i] = bi
            if mp["flags"][i] & 2: closed[bi] = 1
    return m, nm, choice, stats


def three_maxima(hist):
    ind, mx = [-1, -1, -1], [0, 0, 0]
    for i, s in enumerate(hist):
        if s > mx[0]: mx = [s, mx[0], mx[1]]; ind = [i, ind[0], ind[1]]
        elif s > mx[1]: mx = [mx[0], s, mx[1]]; ind = [ind[0], i, ind[1]]
        elif s > mx[2]: mx[2] = s; ind[2] = i
    if f32(mx[1]) < f32(f32(0.1) * f32(mx[0])): ind[1] = ind[2] = -1
    elif f32(mx[2]) < f32(f32(0.1) * f32(mx[0])): ind[2] = -1
    return ind


def search_kf(cam, sc, T, kf, cur, th, orb_dist, check_orientation=True):
    fx, fy, cx, cy = [f32(v) for v in cam[:4]]; b = [f32(v) for v in cam[6:10]]; th = f32(th)
    T = np.asarray(T, np.float32); Ow = camera_centre(T)
    n_cur = len(cur["octave"])
    holds = np.zeros(n_cur, np.uint8) if cur.get("taken") is None else np.array(cur["taken"], np.uint8)
    m = np.full(n_cur, -1, np.int32); nm = 0; rot_hist = [[] for _ in range(HISTO_LENGTH)]; factor = f32(f32(1.0) / f32(HISTO_LENGTH))
    for i in range(len(kf["valid"])):
        if not kf["valid"][i]: continue
        P = kf["x3Dw"][i]
        Pc = to_camera(T, P)
        invzc = f32(f64(1.0) / f64(Pc[2]))
        u = f32(f32(f32(fx * Pc[0]) * invzc) + cx); v = f32(f32(f32(fy * Pc[1]) * invzc) + cy)
        if u < b[0] or u > b[1]: continue
        if v < b[2] or v > b[3]: continue
        _, dist = distance(P, Ow)
        if dist < f32(f32(0.8) * kf["min_dist"][i]) or dist > f32(f32(1.2) * kf["max_dist"][i]): continue
        lv = predict_scale(kf["max_dist"][i], dist, sc)
        bd, bi = 256, -1
        for k in features_in_area(cam, cur, u, v, f32(th * sc[lv]), lv - 1, lv + 1):
            if holds[k]: continue
            d = hamming(kf["desc"][i], cur["desc"][k])
            if d < bd: bd, bi = d, k
        if bd <= orb_dist:
            m[bi] = i; holds[bi] = 1; nm += 1
            if check_orientation:
                rot = f32(kf["angle"][i] - cur["angle"][bi])
                if rot < 0: rot = f32(rot + f32(360.0))
                bn = int(np.floor(f64(f32(rot * factor)) + 0.5))            # round(): halves away from zero, the product is never negative
                rot_hist[0 if bn == HISTO_LENGTH else bn].append(bi)
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist])
        for bn in range(HISTO_LENGTH):
            if bn not in keep:
                for k in rot_hist[bn]:
                    m[k] = -1; nm -= 1
    return m, nm
