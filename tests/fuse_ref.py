"""Plain Python restatement of the reference's projections of map points into a key frame (test infrastructure; nothing under sindslam_amd/ imports it):
  fuse_search()     the search of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:825-949) and of Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:977-1079),
  search_kf_sim3()  ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:290-403),
  search_by_sim3()  ORBmatcher::SearchBySim3 (:1102-1326),
  kf_features_in_area()  KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:569-608) on the CSR grid, with the key frame's int bounds (include/KeyFrame.h:185-188),
  Graph, fuse_full(), fuse_replay()  a toy MapPoint / KeyFrame graph, the reference's Fuse loop including its tail (:952-971, :1082-1096) on it, and the caller loop
                    that include/sind_hip.h documents for sind_match_fuse.
Sequential loops, numpy.float32 / float64 scalars placed where the reference (and the OpenCV 4.2.0 calls it makes) round; the small-matrix algebra as
sindslam_amd/csrc/match_local.hip (1)-(7) defines it.  cam10 as match_scene builds it.  A key frame is a dict: un_xy, octave, u_right, desc, grid_start, grid_idx."""
import copy

import numpy as np

import localmap_ref as R
from localmap_ref import BEHIND, IN_VIEW, NOT_CANDIDATE, OUT_ANGLE, OUT_DIST, OUT_X, OUT_Y, f32, f64, hamming

TH_LOW, TH_HIGH = 50, 100
FUSE, FUSE_SIM3, PROJ_SIM3, BY_SIM3 = 0, 1, 2, 3


def kf_bounds(cam):
    """(mnMinX, mnMaxX, mnMinY, mnMaxY) as the KeyFrame keeps them (int: truncated), mfGridElementWidthInv, mfGridElementHeightInv (the frame's, from its float bounds)"""
    b = [f32(v) for v in cam[6:10]]
    return [f32(np.trunc(v)) for v in b], f32(f32(64) / f32(b[1] - b[0])), f32(f32(48) / f32(b[3] - b[2]))


def kf_features_in_area(cam, kf, x, y, r):
    kb, w_inv, h_inv = kf_bounds(cam)
    x0 = max(0, int(np.floor(f32(f32(f32(x - kb[0]) - r) * w_inv))))
    if x0 >= 64: return []
    x1 = min(63, int(np.ceil(f32(f32(f32(x - kb[0]) + r) * w_inv))))
    if x1 < 0: return []
    y0 = max(0, int(np.floor(f32(f32(f32(y - kb[2]) - r) * h_inv))))
    if y0 >= 48: return []
    y1 = min(47, int(np.ceil(f32(f32(f32(y - kb[2]) + r) * h_inv))))
    if y1 < 0: return []
    gs, gi, xy = kf["grid_start"], kf["grid_idx"], kf["un_xy"]
    out = []
    for ix in range(x0, x1 + 1):
        for j in range(gs[ix * 48 + y0], gs[ix * 48 + y1 + 1]):            # cells (ix, y0..y1) are contiguous in the CSR
            k = gi[j]
            if abs(f32(xy[k, 0] - x)) < r and abs(f32(xy[k, 1] - y)) < r: out.append(int(k))
    return out


def decompose_scw(S):
    """Scw -> 4x4 [Rcw | tcw] (:298-302, :986-989): scw = (float)sqrt(row0 . row0) accumulated in FP64, every element times (float)(1.0 / scw) in FP32"""
    S = np.asarray(S, np.float32)
    scw = f32(np.sqrt(sum(f64(S[0, k]) * f64(S[0, k]) for k in range(3))))
    T = np.eye(4, dtype=np.float32); T[:3] = S[:3] * f32(f64(1.0) / f64(scw))
    return T


def sim3_transforms(s12, R12, t12):
    """([sR21 | t21], [sR12 | t12]) as 3x4 (:1119-1121): s12 * R12 and (1.0 / s12) * R12^T in FP32, t21 = -sR21 * t12 as an FP32 row product times -1.0 in FP64"""
    R12 = np.asarray(R12, np.float32); t12 = np.asarray(t12, np.float32); s12 = f32(s12)
    T12 = np.zeros((3, 4), np.float32); T21 = np.zeros((3, 4), np.float32)
    T12[:, :3] = R12 * s12; T12[:, 3] = t12
    T21[:, :3] = R12.T * f32(f64(1.0) / f64(s12))
    for r in range(3):
        t = f32(f32(f32(T21[r, 0] * t12[0]) + f32(T21[r, 1] * t12[1])) + f32(T21[r, 2] * t12[2]))
        T21[r, 3] = f32(f64(t) * f64(-1.0))
    return T21, T12


def project(mode, cam, sc, T, Ow, P, Pn, max_dist, min_dist, T2=None):
    """one point up to GetFeaturesInArea -> (why, u, v, invz, level); why != IN_VIEW: the `continue` it left by (IsInImage is one test: OUT_X is reported first)"""
    fx, fy, cx, cy = [f32(v) for v in cam[:4]]
    kb = kf_bounds(cam)[0]
    Pc = R.to_camera(T, P)
    if mode == BY_SIM3: Pc = R.to_camera(T2, Pc)
    if Pc[2] < 0: return BEHIND, None, None, None, None                     # < 0.0f and < 0.0 agree on a float
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = f32(f32(1.0) / Pc[2]) if mode in (FUSE, PROJ_SIM3) else f32(f64(1.0) / f64(Pc[2]))
        u = f32(f32(fx * f32(Pc[0] * invz)) + cx); v = f32(f32(fy * f32(Pc[1] * invz)) + cy)
    if not (u >= kb[0] and u < kb[1]): return OUT_X, None, None, None, None
    if not (v >= kb[2] and v < kb[3]): return OUT_Y, None, None, None, None
    if mode == BY_SIM3: PO = Pc; dist = f32(np.sqrt(sum(f64(x) * f64(x) for x in PO)))
    else: PO, dist = R.distance(P, Ow)
    if dist < f32(f32(0.8) * min_dist) or dist > f32(f32(1.2) * max_dist): return OUT_DIST, None, None, None, None
    if mode != BY_SIM3 and sum(f64(PO[k]) * f64(Pn[k]) for k in range(3)) < f64(0.5) * f64(dist): return OUT_ANGLE, None, None, None, None
    return IN_VIEW, u, v, invz, R.predict_scale(max_dist, dist, sc)


def chi2_ok(cam, sc, kf, k, u, v, invz):
    """the reprojection test of Fuse(pKF, vpMapPoints) for candidate k (:914-938) -> (passes, stereo)"""
    bf = f32(cam[4]); lvl = int(kf["octave"][k])
    inv_sigma2 = f32(f32(1.0) / f32(sc[lvl] * sc[lvl]))
    ex = f32(u - kf["un_xy"][k, 0]); ey = f32(v - kf["un_xy"][k, 1])
    e2 = f32(f32(ex * ex) + f32(ey * ey))
    stereo = kf["u_right"][k] >= 0
    if stereo:
        er = f32(f32(u - f32(bf * invz)) - kf["u_right"][k])
        e2 = f32(e2 + f32(er * er))
    return not (f64(f32(e2 * inv_sigma2)) > (7.8 if stereo else 5.99)), bool(stereo)


def search_point(mode, cam, sc, kf, th, u, v, invz, lv, desc, closed=None, stats=None):
    """the window walk of one point -> (bestDist, bestIdx): levels [lv-1, lv], strict <, the first of equal distances in walk order"""
    bd, bi = 256, -1
    for k in kf_features_in_area(cam, kf, u, v, f32(f32(th) * sc[lv])):
        if closed is not None and closed[k]: continue
        if kf["octave"][k] < lv - 1 or kf["octave"][k] > lv: continue
        if mode == FUSE:
            ok, stereo = chi2_ok(cam, sc, kf, k, u, v, invz)
            if stats is not None: stats[("stereo" if stereo else "mono") + ("_pass" if ok else "_reject")] += 1
            if not ok: continue
        d = hamming(desc, kf["desc"][k])
        if d < bd: bd, bi = d, k
    return bd, bi


def _pose(T, sim3):
    T = decompose_scw(T) if sim3 else np.asarray(T, np.float32)
    return T, R.camera_centre(T)


def fuse_search(cam, sc, T, mp, kf, th, sim3):
    """-> dict: best_idx, best_dist [n], nfused, why [n], level [n], proj [n, 2], stats (chi-square outcomes per candidate)"""
    mode = FUSE_SIM3 if sim3 else FUSE
    T, Ow = _pose(T, sim3); n = len(mp["valid"])
    out = dict(best_idx=np.full(n, -1, np.int32), best_dist=np.full(n, -1, np.int32), nfused=0, why=np.zeros(n, np.int32), level=np.full(n, -1, np.int32),
               proj=np.zeros((n, 2), np.float32), stats=dict(stereo_pass=0, stereo_reject=0, mono_pass=0, mono_reject=0))
    for i in range(n):
        if not mp["valid"][i]:
            out["why"][i] = NOT_CANDIDATE; continue
        why, u, v, invz, lv = project(mode, cam, sc, T, Ow, mp["x3Dw"][i], mp["normal"][i], mp["max_dist"][i], mp["min_dist"][i])
        out["why"][i] = why
        if why != IN_VIEW: continue
        out["level"][i] = lv; out["proj"][i] = (u, v)
        bd, bi = search_point(mode, cam, sc, kf, th, u, v, invz, lv, mp["desc"][i], stats=out["stats"])
        if bd <= TH_LOW:
            out["best_idx"][i] = bi; out["best_dist"][i] = bd; out["nfused"] += 1
    return out


def search_kf_sim3(cam, sc, Scw, mp, kf, th, sequential=True):
    """-> match_of_kf [n_kf], nmatches, choice [n], why [n].  sequential=False searches every point against vpMatched as it was on entry."""
    T, Ow = _pose(Scw, True); n = len(mp["valid"]); n_kf = len(kf["octave"]); th = f32(int(th))
    closed = np.zeros(n_kf, np.uint8) if kf.get("taken") is None else np.array(kf["taken"], np.uint8)
    closed0 = closed.copy()
    m = np.full(n_kf, -1, np.int32); nm = 0; choice = np.full(n, -1, np.int32); whys = np.zeros(n, np.int32)
    for i in range(n):
        if not mp["valid"][i]:
            whys[i] = NOT_CANDIDATE; continue
        why, u, v, invz, lv = project(PROJ_SIM3, cam, sc, T, Ow, mp["x3Dw"][i], mp["normal"][i], mp["max_dist"][i], mp["min_dist"][i])
        whys[i] = why
        if why != IN_VIEW: continue
        bd, bi = search_point(PROJ_SIM3, cam, sc, kf, th, u, v, invz, lv, mp["desc"][i], closed=closed if sequential else closed0)
        if bd <= TH_LOW:
            choice[i] = bi; nm += 1
            if sequential: m[bi] = i; closed[bi] = 1
    return m, nm, choice, whys


def search_by_sim3(cam, sc, T1w, T2w, s12, R12, t12, side1, side2, th):
    """a side, per slot: valid, x3Dw, max_dist, min_dist, mp_desc, and the slot's keypoint un_xy, octave, kf_desc; grid_start, grid_idx.
    -> match12 [n1], nfound, vnMatch1 [n1], vnMatch2 [n2], why1 [n1], why2 [n2]"""
    T21, T12 = sim3_transforms(s12, R12, t12)
    vn, whys = [], []
    for src, dst, Tw, T2 in ((side1, side2, T1w, T21), (side2, side1, T2w, T12)):
        kf = dict(un_xy=dst["un_xy"], octave=dst["octave"], desc=dst["kf_desc"], grid_start=dst["grid_start"], grid_idx=dst["grid_idx"])
        Tw = np.asarray(Tw, np.float32); n = len(src["valid"]); v12 = np.full(n, -1, np.int32); w = np.zeros(n, np.int32)
        for i in range(n):
            if not src["valid"][i]:
                w[i] = NOT_CANDIDATE; continue
            why, u, v, invz, lv = project(BY_SIM3, cam, sc, Tw, None, src["x3Dw"][i], None, src["max_dist"][i], src["min_dist"][i], T2=T2)
            w[i] = why
            if why != IN_VIEW: continue
            bd, bi = search_point(BY_SIM3, cam, sc, kf, th, u, v, invz, lv, src["mp_desc"][i])
            if bd <= TH_HIGH: v12[i] = bi
        vn.append(v12); whys.append(w)
    m12 = np.full(len(vn[0]), -1, np.int32); nfound = 0
    for i1, idx2 in enumerate(vn[0]):
        if idx2 >= 0 and vn[1][idx2] == i1:
            m12[i1] = idx2; nfound += 1
    return m12, nfound, vn[0], vn[1], whys[0], whys[1]


# ---- a toy object graph for the tail of Fuse ----
class Graph:
    """points[pid]: dict(bad, obs {kf id: keypoint index}, desc, x3Dw, normal, max_dist, min_dist); slots[kf id]: {keypoint index: pid} (KeyFrame::mvpMapPoints, absent =
    NULL); log: what the tails did, in order."""

    def __init__(self):
        self.points, self.slots, self.log = [], {}, []

    def add_point(self, x3Dw, normal, max_dist, min_dist, desc, bad=False):
        self.points.append(dict(bad=bad, obs={}, desc=np.array(desc, np.uint8), x3Dw=np.array(x3Dw, np.float32), normal=np.array(normal, np.float32), max_dist=f32(max_dist), min_dist=f32(min_dist)))
        return len(self.points) - 1

    def observe(self, pid, kf_id, idx):
        """MapPoint::AddObservation + KeyFrame::AddMapPoint"""
        self.points[pid]["obs"][kf_id] = idx; self.slots.setdefault(kf_id, {})[idx] = pid

    def n_obs(self, pid):
        return len(self.points[pid]["obs"])

    def replace(self, loser, survivor):
        """points[loser].Replace(points[survivor]) (src/MapPoint.cc:177-213): the observations move, the loser turns bad, the survivor's descriptor is recomputed
        (here: a fixed function of both, so that it changes)"""
        if loser == survivor: return
        a, b = self.points[loser], self.points[survivor]
        obs, a["obs"], a["bad"] = a["obs"], {}, True
        for kf_id, idx in obs.items():
            if kf_id not in b["obs"]:
                self.slots[kf_id][idx] = survivor; b["obs"][kf_id] = idx
            else:
                del self.slots[kf_id][idx]
        b["desc"] = np.bitwise_xor(b["desc"], np.roll(a["desc"], 1))
        self.log.append(("replace", loser, survivor))

    def state(self):
        return ([(p["bad"], sorted(p["obs"].items()), p["desc"].tobytes()) for p in self.points], {k: sorted(v.items()) for k, v in self.slots.items()})

    def inputs(self, kf_id, plist, sim3):
        """the flat arrays of sind_match_fuse for this list as the graph is now (plist entry -1 = NULL); spAlreadyFound (sim3) is the key frame's points now"""
        found = set(self.slots.get(kf_id, {}).values())
        pts = [self.points[max(p, 0)] for p in plist]
        valid = [p >= 0 and not self.points[p]["bad"] and ((p not in found) if sim3 else (kf_id not in self.points[p]["obs"])) for p in plist]
        return dict(x3Dw=np.array([p["x3Dw"] for p in pts], np.float32).reshape(-1, 3), normal=np.array([p["normal"] for p in pts], np.float32).reshape(-1, 3),
                    max_dist=np.array([p["max_dist"] for p in pts], np.float32), min_dist=np.array([p["min_dist"] for p in pts], np.float32),
                    desc=np.array([p["desc"] for p in pts], np.uint8).reshape(-1, 32), valid=np.array(valid, np.uint8))


def _tail(g, kf_id, pid, best, sim3, replace_point, i):
    """:952-971 (sim3 = 0) and :1082-1096 (sim3 = 1) for point pid and keypoint best"""
    pin = g.slots.get(kf_id, {}).get(best, -1)
    if pin >= 0:
        if not g.points[pin]["bad"]:
            if sim3: replace_point[i] = pin
            elif g.n_obs(pin) > g.n_obs(pid): g.replace(pid, pin)
            else: g.replace(pin, pid)
        else:
            g.log.append(("bad_in_kf", pid, pin))
    else:
        g.observe(pid, kf_id, best); g.log.append(("add", pid, best))


def fuse_full(g, cam, sc, T, kf_id, kf, plist, th, sim3):
    """the reference's loop on the live graph -> (nFused, vpReplacePoint as pids, -1 = NULL)"""
    mode = FUSE_SIM3 if sim3 else FUSE
    Tm, Ow = _pose(T, sim3); n = 0; replace_point = [-1] * len(plist)
    found = set(g.slots.get(kf_id, {}).values())                           # spAlreadyFound: a snapshot in the reference too (:993)
    for i, pid in enumerate(plist):
        if pid < 0: continue
        p = g.points[pid]
        if p["bad"] or ((pid in found) if sim3 else (kf_id in p["obs"])): continue
        why, u, v, invz, lv = project(mode, cam, sc, Tm, Ow, p["x3Dw"], p["normal"], p["max_dist"], p["min_dist"])
        if why != IN_VIEW: continue
        bd, bi = search_point(mode, cam, sc, kf, th, u, v, invz, lv, p["desc"])
        if bd <= TH_LOW:
            _tail(g, kf_id, pid, bi, sim3, replace_point, i); n += 1
    return n, replace_point


def fuse_replay(g, best_idx, kf_id, plist, sim3):
    """the caller's loop after sind_match_fuse: in point order; for sim3 = 0 the re-test of isBad() || IsInKeyFrame(pKF) first"""
    n = 0; replace_point = [-1] * len(plist)
    for i, pid in enumerate(plist):
        if best_idx[i] < 0: continue
        if not sim3 and (g.points[pid]["bad"] or kf_id in g.points[pid]["obs"]): continue
        _tail(g, kf_id, pid, int(best_idx[i]), sim3, replace_point, i); n += 1
    return n, replace_point


def clone(g):
    return copy.deepcopy(g)
