"""Plain Python/NumPy restatement of the map-point arithmetic, written from the reference's lines: the per-match loop of LocalMapping::CreateNewMapPoints
(src/LocalMapping.cc:284-431) with KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631), MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and
MapPoint::UpdateNormalAndDepth (:330-371).  Every step is an explicit np.float32 or np.float64 operation in the order and type csrc/host/map_points.hpp states, with its
own Jacobi SVD (OpenCV 4.2's JacobiSVDImpl_<float> as remembered), so the host twins equal it bit for bit by construction.  atan2 and cos of the stereo parallax are the C
library's float functions, as in the library."""
import ctypes as C
import ctypes.util

import numpy as np

F, D = np.float32, np.float64
FLT_EPSILON = F(1.1920928955078125e-07)
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = C.c_float; _libm.atan2f.argtypes = [C.c_float, C.c_float]
_libm.cosf.restype = C.c_float; _libm.cosf.argtypes = [C.c_float]
STATUS = dict(new=0, low_parallax=1, w0=2, z1=3, z2=4, reproj1=5, reproj2=6, dist0=7, scale=8)


def stereo_cos(mb, depth):
    """cos(2 * atan2(mb / 2, depth)) with the float overloads (:312, :314)"""
    return F(_libm.cosf(float(F(2) * F(_libm.atan2f(float(F(mb) / F(2)), float(F(depth)))))))


def hypot(a, b):
    a = abs(D(a)); b = abs(D(b))
    if a > b:
        b = b / a
        return a * np.sqrt(D(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(D(1) + a * a)
    return D(0)


def dot3(a, b):
    s = D(0)
    for k in range(3):
        s = s + D(a[k]) * D(b[k])
    return s


def norm3(a):
    return np.sqrt(dot3(a, a))


def svd4_last_row(At):
    """JacobiSVDImpl_<float>(At, W, Vt, 4, 4, 4): At = A^T as a list of four lists of np.float32 -> row 3 of Vt after the descending sort"""
    eps = FLT_EPSILON * F(2)
    Vt = [[F(1) if i == k else F(0) for k in range(4)] for i in range(4)]
    W = [D(0)] * 4
    for i in range(4):
        sd = D(0)
        for k in range(4):
            sd = sd + D(At[i][k]) * D(At[i][k])
        W[i] = sd
    for _ in range(30):
        changed = False
        for i in range(3):
            for j in range(i + 1, 4):
                Ai, Aj = At[i], At[j]
                a, p, b = W[i], D(0), W[j]
                for k in range(4):
                    p = p + D(Ai[k]) * D(Aj[k])
                if abs(p) <= D(eps) * np.sqrt(a * b):
                    continue
                p = p * D(2)
                beta = a - b; gamma = hypot(p, beta)
                if beta < 0:
                    delta = (gamma - beta) * D(0.5)
                    s = F(np.sqrt(delta / gamma)); c = F(p / (gamma * D(s) * D(2)))
                else:
                    c = F(np.sqrt((gamma + beta) / (gamma * D(2)))); s = F(p / (gamma * D(c) * D(2)))
                a = b = D(0)
                for k in range(4):
                    t0 = c * Ai[k] + s * Aj[k]; t1 = (-s) * Ai[k] + c * Aj[k]
                    Ai[k] = t0; Aj[k] = t1
                    a = a + D(t0) * D(t0); b = b + D(t1) * D(t1)
                W[i] = a; W[j] = b
                changed = True
                Vi, Vj = Vt[i], Vt[j]
                for k in range(4):
                    t0 = c * Vi[k] + s * Vj[k]; t1 = (-s) * Vi[k] + c * Vj[k]
                    Vi[k] = t0; Vj[k] = t1
        if not changed:
            break
    for i in range(4):
        sd = D(0)
        for k in range(4):
            sd = sd + D(At[i][k]) * D(At[i][k])
        W[i] = np.sqrt(sd)
    for i in range(3):
        j = i
        for k in range(i + 1, 4):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]; Vt[i], Vt[j] = Vt[j], Vt[i]
    return Vt[3]


def camera(K5, scale):
    fx, fy, cx, cy, bf = [F(v) for v in K5]
    scale = [F(s) for s in scale]
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, invfx=F(1) / fx, invfy=F(1) / fy, mb=bf / fx, scale=scale, sigma2=[s * s for s in scale], ratioFactor=F(1.5) * scale[1])


def triangulation_matrix(c, T1, T2, un1, un2):
    """A of :322-326 (rows), from xn1, xn2 and the two poses"""
    xn1 = [(F(un1[0]) - c["cx"]) * c["invfx"], (F(un1[1]) - c["cy"]) * c["invfy"], F(1)]
    xn2 = [(F(un2[0]) - c["cx"]) * c["invfx"], (F(un2[1]) - c["cy"]) * c["invfy"], F(1)]
    A = [[T1[2][k] * xn1[0] - T1[0][k] for k in range(4)], [T1[2][k] * xn1[1] - T1[1][k] for k in range(4)],
         [T2[2][k] * xn2[0] - T2[0][k] for k in range(4)], [T2[2][k] * xn2[1] - T2[1][k] for k in range(4)]]
    return xn1, xn2, A


def cos_parallax_rays(c, T1, T2, un1, un2):
    """cosParallaxRays of :300-305: ray = Rwc * xn with Rwc the transpose of Tcw's rotation"""
    xn1, xn2, _ = triangulation_matrix(c, T1, T2, un1, un2)
    ray1 = [T1[0][r] * xn1[0] + T1[1][r] * xn1[1] + T1[2][r] * xn1[2] for r in range(3)]
    ray2 = [T2[0][r] * xn2[0] + T2[1][r] * xn2[1] + T2[2][r] * xn2[2] for r in range(3)]
    return F(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)))


def unproject_stereo(c, Twc, xy, z):
    x = (F(xy[0]) - c["cx"]) * z * c["invfx"]; y = (F(xy[1]) - c["cy"]) * z * c["invfy"]
    out = []
    for r in range(3):
        t = Twc[r][0] * x + Twc[r][1] * y + Twc[r][2] * z
        out.append(F(D(t) * D(1) + D(Twc[r][3]) * D(1)))
    return out


def tri_point(c, T1, W1, T2, W2, k1, k2):
    """one pass of :286-450 up to `new MapPoint`.  T = Tcw, W = Twc as [4][4] np.float32; k = (un_xy, xy, u_right, depth, octave) -> (x3D, how, status)"""
    zero = [F(0)] * 3
    (un1, xy1, ur1, dp1, o1), (un2, xy2, ur2, dp2, o2) = k1, k2
    ur1, ur2, dp1, dp2 = F(ur1), F(ur2), F(dp1), F(dp2)
    st1, st2 = ur1 >= 0, ur2 >= 0
    xn1, xn2, A = triangulation_matrix(c, T1, T2, un1, un2)
    cosRays = cos_parallax_rays(c, T1, T2, un1, un2)
    cs1 = cs2 = cosRays + F(1)
    if st1:
        cs1 = stereo_cos(c["mb"], dp1)
    elif st2:
        cs2 = stereo_cos(c["mb"], dp2)
    cs = cs2 if cs2 < cs1 else cs1
    if cosRays < cs and cosRays > 0 and (st1 or st2 or D(cosRays) < D(0.9998)):
        At = [[A[r][k] for r in range(4)] for k in range(4)]
        x = svd4_last_row(At)
        if x[3] == 0:
            return zero, 0, STATUS["w0"]
        inv = F(D(1) / D(x[3]))
        X = [x[k] * inv for k in range(3)]; how = 0
    elif st1 and cs1 < cs2:
        X = unproject_stereo(c, W1, xy1, dp1); how = 1
    elif st2 and cs2 < cs1:
        X = unproject_stereo(c, W2, xy2, dp2); how = 2
    else:
        return zero, -1, STATUS["low_parallax"]
    z1 = F(dot3(T1[2], X) + D(T1[2][3]))
    if z1 <= 0:
        return X, how, STATUS["z1"]
    z2 = F(dot3(T2[2], X) + D(T2[2][3]))
    if z2 <= 0:
        return X, how, STATUS["z2"]
    for T, z, un, ur, st, o, code in ((T1, z1, un1, ur1, st1, o1, "reproj1"), (T2, z2, un2, ur2, st2, o2, "reproj2")):
        s2 = c["sigma2"][o]
        x = F(dot3(T[0], X) + D(T[0][3])); y = F(dot3(T[1], X) + D(T[1][3]))
        invz = F(D(1) / D(z))
        u = c["fx"] * x * invz + c["cx"]; v = c["fy"] * y * invz + c["cy"]
        ex = u - F(un[0]); ey = v - F(un[1])
        if not st:
            if D(ex * ex + ey * ey) > D(5.991) * D(s2):
                return X, how, STATUS[code]
        else:
            er = (u - c["bf"] * invz) - ur
            if D(ex * ex + ey * ey + er * er) > D(7.8) * D(s2):
                return X, how, STATUS[code]
    dist1 = F(norm3([X[k] - W1[k][3] for k in range(3)])); dist2 = F(norm3([X[k] - W2[k][3] for k in range(3)]))
    if dist1 == 0 or dist2 == 0:
        return X, how, STATUS["dist0"]
    ratioDist = dist2 / dist1; ratioOctave = c["scale"][o1] / c["scale"][o2]
    if ratioDist * c["ratioFactor"] < ratioOctave or ratioDist > ratioOctave * c["ratioFactor"]:
        return X, how, STATUS["scale"]
    return X, how, STATUS["new"]


def triangulate(pairs, K5, scale):
    """what ORBmatcher.Triangulate returns, for the same pairs"""
    c = camera(K5, scale); out = []
    with np.errstate(all="ignore"):
        for p in pairs:
            T = {k: [[F(v) for v in row] for row in np.asarray(p[k], np.float32).reshape(4, 4)] for k in ("Tcw1", "Twc1", "Tcw2", "Twc2")}
            k1, k2 = p["kf1"], p["kf2"]; n1 = len(k1["octave"])
            x3D = np.zeros((n1, 3), np.float32); how = np.full(n1, -1, np.int32); status = np.full(n1, -1, np.int32)
            for i, j in enumerate(np.asarray(p["match12"]).tolist()):
                if j < 0:
                    continue
                side = lambda k, a: (np.asarray(k["un_xy"], np.float32)[a], np.asarray(k["xy"], np.float32)[a], k["u_right"][a], k["depth"][a], int(k["octave"][a]))
                X, how[i], status[i] = tri_point(c, T["Tcw1"], T["Twc1"], T["Tcw2"], T["Twc2"], side(k1, i), side(k2, j))
                x3D[i] = X
            out.append(dict(x3D=x3D, how=how, status=status, nnew=int((status == 0).sum())))
    return out


def distinctive_descriptor(desc, bad):
    """ComputeDistinctiveDescriptors as written.  desc u8 [n, 32], bad [n] -> position in the list of the chosen descriptor, or -1 (mDescriptor stays)"""
    v = [e for e in range(len(desc)) if not bad[e]]
    if not v:
        return -1
    bits = np.unpackbits(np.asarray(desc, np.uint8)[v], axis=1).astype(np.int32)
    N = len(v)
    Distances = np.zeros((N, N), np.float32)
    for i in range(N):
        for j in range(i + 1, N):
            Distances[i, j] = Distances[j, i] = int((bits[i] != bits[j]).sum())
    BestMedian, BestIdx = 2 ** 31 - 1, 0
    for i in range(N):
        vDists = sorted(int(d) for d in Distances[i])
        median = vDists[int(0.5 * (N - 1))]
        if median < BestMedian:
            BestMedian, BestIdx = median, i
    return v[BestIdx]


def normal_and_depth(P, Ows, ref, octave, scale):
    """UpdateNormalAndDepth.  P [3], Ows = the camera centres of the observers in list order, ref = the position of mpRefKF, octave = its keypoint's -> normal [3], max, min"""
    N = [F(0)] * 3
    P = [F(v) for v in P]
    for O in Ows:
        d = [P[k] - F(O[k]) for k in range(3)]
        inv = F(D(1) / norm3(d))
        N = [d[k] * inv + N[k] for k in range(3)]
    pc = [P[k] - F(Ows[ref][k]) for k in range(3)]
    dist = F(norm3(pc))
    maxD = dist * F(scale[octave]); minD = maxD / F(scale[len(scale) - 1])
    invn = F(D(1) / D(len(Ows)))
    return [N[k] * invn for k in range(3)], maxD, minD


def update_points(items, scale):
    """what ORBmatcher.UpdateMapPoints returns, for the same items"""
    out = []
    with np.errstate(all="ignore"):
        for it in items:
            n = len(it["x3Dw"]); s = np.asarray(it["obs_start"])
            prior = lambda key, shape, dtype: np.array(it[key], dtype).reshape(shape).copy() if it.get(key) is not None else np.zeros(shape, dtype)
            r = dict(desc=prior("desc", (n, 32), np.uint8), best_obs=np.full(n, -1, np.int32), normal=prior("normal", (n, 3), np.float32), max_dist=prior("max_dist", (n,), np.float32),
                     min_dist=prior("min_dist", (n,), np.float32), updated=np.zeros(n, np.uint8))
            desc = np.asarray(it["obs_desc"], np.uint8).reshape(-1, 32)
            for j in range(n):
                a, b = int(s[j]), int(s[j + 1])
                if it.get("do_descriptor", True):
                    r["best_obs"][j] = best = distinctive_descriptor(desc[a:b], it["obs_bad"][a:b])
                    if best >= 0:
                        r["desc"][j] = desc[a + best]
                if it.get("do_normal", True) and b > a:
                    ref = int(it["ref_obs"][j])
                    nv, mx, mn = normal_and_depth(it["x3Dw"][j], [it["Ow"][k] for k in it["obs_kf"][a:b]], ref, int(it["obs_octave"][a + ref]), scale)
                    r["normal"][j] = nv; r["max_dist"][j] = mx; r["min_dist"][j] = mn; r["updated"][j] = 1
            out.append(r)
    return out
