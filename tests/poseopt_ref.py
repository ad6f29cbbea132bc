"""Optimizer::PoseOptimization (reference src/Optimizer.cc:239-451) restated in Python with NumPy FP64 (and FP32) scalars, operation for operation as
sindslam_amd/csrc/host/pose_opt.hpp has it, the defined sin / cos included; the header's head lists what is unpinned against a real g2o / Eigen build.
Bit equality with the host library is BY CONSTRUCTION of the two texts; tests/test_poseopt_cpu.py asserts it and checks the result against things that are neither."""
from __future__ import annotations

import numpy as np

F = np.float64
f32 = np.float32
DBL_MAX = F(np.finfo(np.float64).max)
ZERO, ONE, TWO, HALF = F(0.0), F(1.0), F(2.0), F(0.5)


def sincos(x):
    x = F(x)
    invpio2, pio2_1, pio2_2, pio2_2t = F(6.36619772367581382433e-01), F(1.57079632673412561417e+00), F(6.07710050630396597660e-11), F(2.02226624879595063154e-21)
    fn = np.rint(x * invpio2)
    t = x - fn * pio2_1
    w = fn * pio2_2
    r = t - w
    w = fn * pio2_2t - ((t - r) - w)
    y0 = r - w; y1 = (r - y0) - w
    z = y0 * y0
    S1, S2, S3, S4, S5, S6 = (F(v) for v in (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10))
    v = z * y0; rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    ks = y0 - ((z * (HALF * y1 - v * rs) - y1) - v * S1)
    C1, C2, C3, C4, C5, C6 = (F(v) for v in (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11))
    rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    hz = HALF * z; wc = ONE - hz
    kc = wc + (((ONE - wc) - hz) + (z * rc - y0 * y1))
    q = fn - F(4.0) * np.rint(fn * F(0.25))
    if q == 0.0:
        return ks, kc
    if q == 1.0:
        return kc, -ks
    if q == -1.0:
        return -kc, ks
    return -ks, -kc


def quat_from_matrix(m):
    q = [ZERO] * 4
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0.0:
        t = np.sqrt(t + ONE); q[3] = HALF * t; t = HALF / t
        q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i][i] - m[j][j] - m[k][k] + ONE)
        q[i] = HALF * t; t = HALF / t
        q[3] = (m[k][j] - m[j][k]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[k] = (m[k][i] + m[i][k]) * t
    return q


def quat_to_matrix(q):
    tx, ty, tz = TWO * q[0], TWO * q[1], TWO * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz, tyy, tyz, tzz = tx * q[0], ty * q[0], tz * q[0], ty * q[1], tz * q[1], tz * q[2]
    return [[ONE - (tyy + tzz), txy - twz, txz + twy], [txy + twz, ONE - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, ONE - (txx + tyy)]]


def quat_rotate(q, v):
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [u + u for u in uv]
    return [v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]), v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]), v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0])]


def normalize_rotation(q):
    if q[3] < 0.0:
        q = [c * F(-1.0) for c in q]
    nrm = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / nrm for c in q]


def se3(R, t):
    return (normalize_rotation(quat_from_matrix(R)), list(t))


def from_tcw(T):
    T = np.asarray(T, np.float32).reshape(4, 4)
    return se3([[F(T[i, j]) for j in range(3)] for i in range(3)], [F(T[i, 3]) for i in range(3)])


def to_tcw(P):
    R = quat_to_matrix(P[0])
    T = np.zeros((4, 4), np.float32)
    for i in range(3):
        for j in range(3):
            T[i, j] = f32(R[i][j])
        T[i, 3] = f32(P[1][i])
    T[3, 3] = 1.0
    return T


def se3_map(P, X):
    r = quat_rotate(P[0], X)
    return [r[0] + P[1][0], r[1] + P[1][1], r[2] + P[1][2]]


def se3_exp(u):
    om, up = u[:3], u[3:]
    theta = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    O = [[ZERO, -om[2], om[1]], [om[2], ZERO, -om[0]], [-om[1], om[0], ZERO]]
    O2 = [[O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
    I = lambda i, j: ONE if i == j else ZERO
    if theta < 0.00001:
        R = [[(I(i, j) + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        s, c = sincos(theta)
        a = s / theta; b = (ONE - c) / (theta * theta); d = (theta - s) / (theta * theta * theta)
        R = [[(I(i, j) + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]
        V = [[(I(i, j) + b * O[i][j]) + d * O2[i][j] for j in range(3)] for i in range(3)]
    t = [V[i][0] * up[0] + V[i][1] * up[1] + V[i][2] * up[2] for i in range(3)]
    return (normalize_rotation(quat_from_matrix(R)), t)


def se3_mul(A, B):
    rt = quat_rotate(A[0], B[1])
    a, b = A[0], B[0]
    t = [A[1][0] + rt[0], A[1][1] + rt[1], A[1][2] + rt[2]]
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    return (normalize_rotation([x, y, z, w]), t)


def oplus(u, est):
    return se3_mul(se3_exp(u), est)


def edge_error(P, K, X, ox, oy, uR, stereo, s):
    """-> chi2, e [3], Xc [3]"""
    fx, fy, cx, cy, bf = K
    Xc = se3_map(P, X)
    if not stereo:
        px = Xc[0] / Xc[2]; py = Xc[1] / Xc[2]
        e = [ox - (px * fx + cx), oy - (py * fy + cy), ZERO]
        return e[0] * (s * e[0]) + e[1] * (s * e[1]), e, Xc
    invz = F(f32(ONE / Xc[2]))
    r0 = Xc[0] * invz * fx + cx; r1 = Xc[1] * invz * fy + cy; r2 = r0 - bf * invz
    e = [ox - r0, oy - r1, uR - r2]
    return e[0] * (s * e[0]) + e[1] * (s * e[1]) + e[2] * (s * e[2]), e, Xc


def huber(e, delta):
    dsqr = delta * delta
    if e <= dsqr:
        return e, ONE
    sqrte = np.sqrt(e)
    return TWO * sqrte * delta - dsqr, delta / sqrte


DELTA = {False: F(f32(np.sqrt(F(5.991)))), True: F(f32(np.sqrt(F(7.815))))}


def edge_contrib(P, K, edge, robust, full):
    """-> c [28] (not full: only c[27] is set)"""
    fx, fy, cx, cy, bf = K
    X, ox, oy, uR, s, stereo = edge
    chi2, e, Xc = edge_error(P, K, X, ox, oy, uR, stereo, s)
    rho0, rho1 = (chi2, ONE)
    if robust:
        rho0, rho1 = huber(chi2, DELTA[stereo])
    c = [ZERO] * 28
    c[27] = rho0
    if not full:
        return c
    x, y = Xc[0], Xc[1]; invz = ONE / Xc[2]; invz_2 = invz * invz
    A = [[x * y * invz_2 * fx, -(ONE + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, ZERO, x * invz_2 * fx],
         [(ONE + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, ZERO, -invz * fy, y * invz_2 * fy], [ZERO] * 6]
    if stereo:
        A[2] = [A[0][0] - bf * y * invz_2, A[0][1] + bf * x * invz_2, A[0][2], A[0][3], ZERO, A[0][5] - bf * invz_2]
    W = rho1 * s if robust else s
    se = [s * e[0], s * e[1], s * e[2]]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            h = (A[0][i] * W) * A[0][j] + (A[1][i] * W) * A[1][j]
            if stereo:
                h = h + (A[2][i] * W) * A[2][j]
            c[k] = h; k += 1
    for j in range(6):
        t = A[0][j] * se[0] + A[1][j] * se[1]
        if stereo:
            t = t + A[2][j] * se[2]
        c[21 + j] = rho1 * t if robust else t
    return c


def edge_is_outlier(P, K, edge):
    X, ox, oy, uR, s, stereo = edge
    chi2 = f32(edge_error(P, K, X, ox, oy, uR, stereo, s)[0])
    return bool(chi2 > (f32(7.815) if stereo else f32(5.991)))


def ldlt_solve(H, b, x):
    """-> (ok, x): x unchanged if not ok"""
    m = [row[:] for row in H]; tr = [0] * 6; temp = [ZERO] * 6
    sign = 0
    for k in range(6):
        big = k; best = abs(m[k][k])
        for i in range(k + 1, 6):
            if abs(m[i][i]) > best:
                best = abs(m[i][i]); big = i
        tr[k] = big
        if k != big:
            for j in range(k):
                m[k][j], m[big][j] = m[big][j], m[k][j]
            for i in range(big + 1, 6):
                m[i][k], m[i][big] = m[i][big], m[i][k]
            m[k][k], m[big][big] = m[big][big], m[k][k]
            for i in range(k + 1, big):
                m[i][k], m[big][i] = m[big][i], m[i][k]
        rs = 6 - k - 1
        if k > 0:
            for j in range(k):
                temp[j] = m[j][j] * m[k][j]
            a = ZERO
            for j in range(k):
                a = a + m[k][j] * temp[j]
            m[k][k] = m[k][k] - a
            for i in range(k + 1, 6):
                v = ZERO
                for j in range(k):
                    v = v + m[i][j] * temp[j]
                m[i][k] = m[i][k] - v
        akk = m[k][k]
        valid = bool(abs(akk) > 0.0)
        if k == 0 and not valid:
            sign = 0; tr = list(range(6)); break
        if rs > 0 and valid:
            for i in range(k + 1, 6):
                m[i][k] = m[i][k] / akk
        if sign == 1:
            if akk < 0.0:
                sign = 2
        elif sign == -1:
            if akk > 0.0:
                sign = 2
        elif sign == 0:
            if akk > 0.0:
                sign = 1
            elif akk < 0.0:
                sign = -1
    if not (sign == 1 or sign == 0):
        return False, x
    d = list(b)
    for k in range(6):
        d[k], d[tr[k]] = d[tr[k]], d[k]
    for j in range(6):
        for i in range(j + 1, 6):
            d[i] = d[i] - d[j] * m[i][j]
    tol = ONE / DBL_MAX
    for i in range(6):
        d[i] = d[i] / m[i][i] if abs(m[i][i]) > tol else ZERO
    for j in range(5, -1, -1):
        for i in range(j - 1, -1, -1):
            d[i] = d[i] - d[j] * m[j][i]
    for k in range(5, -1, -1):
        d[k], d[tr[k]] = d[tr[k]], d[k]
    return True, d


def sums(P, K, edges, outlier, robust, full):
    S = [ZERO] * 28
    for i, e in enumerate(edges):
        if outlier[i]:
            continue
        c = edge_contrib(P, K, e, robust, full)
        if full:
            for k in range(21):
                S[k] = S[k] + c[k]
            for k in range(21, 27):
                S[k] = S[k] - c[k]
        S[27] = S[27] + c[27]
    return S


def pose_optimization(x3Dw, obs_xy, u_right, inv_sigma2, Tcw, K, trace=None):
    """K = fx fy cx cy bf (anything float32 converts).  -> dict of the outputs of sind_poseopt_item (None where the call writes nothing).  trace: a list that gets, per
    linearisation, (round, iteration, iniChi), per trial, (round, iteration, 'trial', tempChi, accepted), and per round (round, 'classified', mvbOutlier after it, the float chi2 it was judged by)"""
    with np.errstate(all="ignore"):
        return _pose_optimization(x3Dw, obs_xy, u_right, inv_sigma2, Tcw, K, trace)


def _pose_optimization(x3Dw, obs_xy, u_right, inv_sigma2, Tcw, K, trace):
    x3Dw = np.asarray(x3Dw, np.float32).reshape(-1, 3); obs_xy = np.asarray(obs_xy, np.float32).reshape(-1, 2)
    u_right = np.asarray(u_right, np.float32).reshape(-1); inv_sigma2 = np.asarray(inv_sigma2, np.float32).reshape(-1)
    n = len(u_right)
    K = [F(f32(k)) for k in K]
    out = dict(n_good=0, n_rounds=0, Tcw=None, outlier=None, round_iters=np.zeros(4, np.int32), round_nbad=np.zeros(4, np.int32), round_pose=np.zeros((4, 12)), round_chi2=np.zeros(4),
               round_lambda=np.zeros(4))
    if n < 3:
        return out
    edges = [([F(x3Dw[i, 0]), F(x3Dw[i, 1]), F(x3Dw[i, 2])], F(obs_xy[i, 0]), F(obs_xy[i, 1]), F(u_right[i]), F(inv_sigma2[i]), not bool(u_right[i] < 0)) for i in range(n)]
    outlier = [False] * n
    P0 = from_tcw(Tcw)
    est = P0
    x = [ZERO] * 6
    lam, ni = F(-1.0), F(2.0)
    nBad = 0
    for it in range(4):
        est = P0; errPose = est
        robust = it < 3
        cj, nBadLM, ok, currentChi = 0, 0, True, ZERO
        i = 0
        while i < 10 and ok:
            S = sums(est, K, edges, outlier, robust, True); errPose = est
            currentChi = S[27]; tempChi = currentChi; iniChi = currentChi
            if trace is not None:
                trace.append((it, i, iniChi))
            H = [[ZERO] * 6 for _ in range(6)]; k = 0
            for a in range(6):
                for c in range(a, 6):
                    H[a][c] = S[k]; H[c][a] = S[k]; k += 1
            b = S[21:27]
            if i == 0:
                maxDiagonal = ZERO
                for j in range(6):
                    a = abs(H[j][j]); maxDiagonal = maxDiagonal if a < maxDiagonal else a
                lam = F(1e-5) * maxDiagonal; ni = F(2.0); nBadLM = 0
            rho = ZERO; qmax = 0
            while True:
                backup = est
                Hl = [[H[a][c] + lam if a == c else H[a][c] for c in range(6)] for a in range(6)]
                ok2, x = ldlt_solve(Hl, b, x)
                est = oplus(x, est)
                T = sums(est, K, edges, outlier, robust, False); errPose = est
                tempChi = T[27]
                if not ok2:
                    tempChi = DBL_MAX
                rho = currentChi - tempChi
                scale = ZERO
                for j in range(6):
                    scale = scale + x[j] * (lam * x[j] + b[j])
                scale = scale + F(1e-3)
                rho = rho / scale
                good = bool(rho > 0 and abs(tempChi) <= DBL_MAX)
                if good:
                    w = TWO * rho - ONE
                    alpha = ONE - w * w * w
                    up, low = F(2.0) / F(3.0), F(1.0) / F(3.0)
                    alpha = up if up < alpha else alpha
                    scaleFactor = alpha if low < alpha else low
                    lam = lam * scaleFactor; ni = F(2.0); currentChi = tempChi
                else:
                    lam = lam * ni; ni = ni * TWO; est = backup
                if trace is not None:
                    trace.append((it, i, "trial", tempChi, good))
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            terminate = False
            if qmax == 10 or rho == 0:
                terminate = True
            else:
                if (iniChi - currentChi) * F(1e3) < iniChi:
                    nBadLM += 1
                else:
                    nBadLM = 0
                if nBadLM >= 3:
                    terminate = True
            ok = not terminate; cj += 1; i += 1
        out["round_iters"][it] = cj; out["round_chi2"][it] = currentChi; out["round_lambda"][it] = lam
        R = quat_to_matrix(est[0])
        out["round_pose"][it] = [R[a][c] for a in range(3) for c in range(3)] + list(est[1])
        new = [edge_is_outlier(est if outlier[k] else errPose, K, e) for k, e in enumerate(edges)]
        if trace is not None:
            trace.append((it, "classified", new, [f32(edge_error(est if outlier[k] else errPose, K, *e[:4], e[5], e[4])[0]) for k, e in enumerate(edges)]))
        outlier = new; nBad = sum(new)
        out["round_nbad"][it] = nBad; out["n_rounds"] = it + 1
        if n < 10:
            break
    out["Tcw"] = to_tcw(est); out["outlier"] = np.array(outlier, np.uint8); out["n_good"] = n - nBad
    return out
