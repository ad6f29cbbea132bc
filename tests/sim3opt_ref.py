"""Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1046-1241) restated in Python with NumPy FP64 scalars, operation for operation as
sindslam_amd/csrc/host/sim3_opt.hpp has it: the defined exp, Sim3's exponential with its four branches, the numeric Jacobian of the two edges, the 7 x 7 LDLT, the two
stages.  The quaternion helpers, sincos and huber are poseopt_ref's (as the header takes them from pose_opt.hpp).  The header's head lists what is unpinned against a
real g2o / Eigen build.  Bit equality with the host library is BY CONSTRUCTION of the two texts; tests/test_sim3opt_cpu.py asserts it and checks the result against
things that are neither."""
from __future__ import annotations

import math

import numpy as np

from poseopt_ref import DBL_MAX, F, HALF, ONE, TWO, ZERO, f32, huber, quat_from_matrix, quat_rotate, sincos

N = 7
DELTA = F(1e-9)


def exp(x):
    x = F(x)
    if not (x == x):
        return x
    if x > 709.782712893384:
        return F(np.inf)
    if x < -745.2:
        return ZERO
    ln2HI, ln2LO, invln2 = F(6.93147180369123816490e-01), F(1.90821492927058770002e-10), F(1.44269504088896338700e+00)
    P1, P2, P3, P4, P5 = (F(v) for v in (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05, -1.65339022054652515390e-06, 4.13813679705723846039e-08))
    fn = np.rint(x * invln2)
    hi = x - fn * ln2HI; lo = fn * ln2LO
    r = hi - lo; t = r * r
    c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    y = ONE - ((lo - (r * c) / (TWO - c)) - hi)
    return F(math.ldexp(float(y), int(fn)))


def from_input(s, R, t):
    """-> Sim3 (q, t, s): Sim3(Matrix3d, Vector3d, double) over the FP32 input"""
    R = np.asarray(R, np.float32).reshape(3, 3); t = np.asarray(t, np.float32).reshape(3)
    return (quat_from_matrix([[F(R[i, j]) for j in range(3)] for i in range(3)]), [F(v) for v in t], F(f32(s)))


def exp7(u):
    om, up, sigma = u[0:3], u[3:6], u[6]
    theta = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    O = [[ZERO, -om[2], om[1]], [om[2], ZERO, -om[0]], [-om[1], om[0], ZERO]]
    s = exp(sigma)
    O2 = [[O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
    eps = F(0.00001)
    small = bool(theta < eps)
    sn, cs = (ZERO, ONE) if small else sincos(theta)
    if abs(sigma) < eps:
        C = ONE
        if small:
            A = ONE / TWO; B = ONE / F(6.0)
        else:
            theta2 = theta * theta
            A = (ONE - cs) / theta2; B = (theta - sn) / (theta2 * theta)
    else:
        C = (s - ONE) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - ONE) * s + ONE) / sigma2
            B = ((HALF * sigma2 - sigma + ONE) * s) / (sigma2 * sigma)
        else:
            a = s * sn; b = s * cs; theta2 = theta * theta; sigma2 = sigma * sigma; c = theta2 + sigma2
            A = (a * sigma + (ONE - b) * theta) / (theta * c)
            B = (C - ((b - ONE) * sigma + a * theta) / c) * ONE / theta2
    I = [[ONE if i == j else ZERO for j in range(3)] for i in range(3)]
    if small:
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
    else:
        ra = sn / theta; rb = (ONE - cs) / (theta * theta)
        R = [[(I[i][j] + ra * O[i][j]) + rb * O2[i][j] for j in range(3)] for i in range(3)]
    q = quat_from_matrix(R)
    t = []
    for i in range(3):
        W = [(A * O[i][j] + B * O2[i][j]) + C * I[i][j] for j in range(3)]
        t.append(W[0] * up[0] + W[1] * up[1] + W[2] * up[2])
    return (q, t, s)


def mul(A, B):
    rt = quat_rotate(A[0], B[1])
    a, b = A[0], B[0]
    q = [ZERO] * 4
    q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    return (q, [A[2] * rt[i] + A[1][i] for i in range(3)], A[2] * B[2])


def inverse(S):
    q = [-S[0][0], -S[0][1], -S[0][2], S[0][3]]
    f = F(-1.0) / S[2]
    return (q, quat_rotate(q, [f * S[1][0], f * S[1][1], f * S[1][2]]), ONE / S[2])


def smap(S, X):
    r = quat_rotate(S[0], X)
    return [S[2] * r[i] + S[1][i] for i in range(3)]


def oplus(u, fix_scale, est):
    """-> (the new estimate, u as oplusImpl leaves it)"""
    u = list(u)
    if fix_scale:
        u[6] = ZERO
    return mul(exp7(u), est), u


def perturbed(est, k, fix_scale):
    S = est
    if k > 0:
        add = [ZERO] * 7
        add[(k - 1) >> 1] = -DELTA if (k - 1) & 1 else DELTA
        S = oplus(add, fix_scale, S)[0]
    return S, inverse(S)


def edge_error(T, K, X, ox, oy, s):
    """-> (chi2, e)"""
    Xc = smap(T, X)
    px = Xc[0] / Xc[2]; py = Xc[1] / Xc[2]
    e = [ox - (px * K[0] + K[2]), oy - (py * K[1] + K[3])]
    return e[0] * (s * e[0]) + e[1] * (s * e[1]), e


def numeric_jacobian(T, K, X, ox, oy, s):
    scalar = ONE / (TWO * DELTA)
    J = [[ZERO] * 7 for _ in range(2)]
    for d in range(7):
        ep = edge_error(T[1 + 2 * d], K, X, ox, oy, s)[1]; em = edge_error(T[2 + 2 * d], K, X, ox, oy, s)[1]
        J[0][d] = scalar * (ep[0] - em[0]); J[1][d] = scalar * (ep[1] - em[1])
    return J


def edge_contrib(T, K, edge, delta, full):
    """edge = (X, ox, oy, s).  -> c [36] (not full: only c[35] is set)"""
    X, ox, oy, s = edge
    chi2, e = edge_error(T[0], K, X, ox, oy, s)
    rho0, rho1 = huber(chi2, delta)
    c = [ZERO] * 36
    c[35] = rho0
    if not full:
        return c
    J = numeric_jacobian(T, K, X, ox, oy, s)
    W = rho1 * s
    omr = [-(s * e[0]), -(s * e[1])]
    omr = [omr[0] * rho1, omr[1] * rho1]
    k = 0
    for i in range(7):
        for j in range(i, 7):
            c[k] = (J[0][i] * W) * J[0][j] + (J[1][i] * W) * J[1][j]; k += 1
    for j in range(7):
        c[28 + j] = J[0][j] * omr[0] + J[1][j] * omr[1]
    return c


def ldlt_solve(H, b, x):
    """-> (ok, x): x unchanged if not ok"""
    m = [row[:] for row in H]; tr = [0] * N; temp = [ZERO] * N
    sign = 0
    for k in range(N):
        big = k; best = abs(m[k][k])
        for i in range(k + 1, N):
            if abs(m[i][i]) > best:
                best = abs(m[i][i]); big = i
        tr[k] = big
        if k != big:
            for j in range(k):
                m[k][j], m[big][j] = m[big][j], m[k][j]
            for i in range(big + 1, N):
                m[i][k], m[i][big] = m[i][big], m[i][k]
            m[k][k], m[big][big] = m[big][big], m[k][k]
            for i in range(k + 1, big):
                m[i][k], m[big][i] = m[big][i], m[i][k]
        rs = N - k - 1
        if k > 0:
            for j in range(k):
                temp[j] = m[j][j] * m[k][j]
            a = ZERO
            for j in range(k):
                a = a + m[k][j] * temp[j]
            m[k][k] = m[k][k] - a
            for i in range(k + 1, N):
                v = ZERO
                for j in range(k):
                    v = v + m[i][j] * temp[j]
                m[i][k] = m[i][k] - v
        akk = m[k][k]
        valid = bool(abs(akk) > 0.0)
        if k == 0 and not valid:
            sign = 0; tr = list(range(N)); break
        if rs > 0 and valid:
            for i in range(k + 1, N):
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
    for k in range(N):
        d[k], d[tr[k]] = d[tr[k]], d[k]
    for j in range(N):
        for i in range(j + 1, N):
            d[i] = d[i] - d[j] * m[i][j]
    tol = ONE / DBL_MAX
    for i in range(N):
        d[i] = d[i] / m[i][i] if abs(m[i][i]) > tol else ZERO
    for j in range(N - 1, -1, -1):
        for i in range(j - 1, -1, -1):
            d[i] = d[i] - d[j] * m[j][i]
    for k in range(N - 1, -1, -1):
        d[k], d[tr[k]] = d[tr[k]], d[k]
    return True, d


class Graph:
    def __init__(self, item, th2, fix_scale):
        g = lambda k, w: np.asarray(item[k], np.float32).reshape(-1, w)
        x1, x2, o1, o2 = g("x3Dc1", 3), g("x3Dc2", 3), g("obs1_xy", 2), g("obs2_xy", 2)
        s1, s2 = g("inv_sigma2_1", 1)[:, 0], g("inv_sigma2_2", 1)[:, 0]
        self.n = len(s1)
        self.K1 = [F(f32(k)) for k in item["K1"]]; self.K2 = [F(f32(k)) for k in item["K2"]]
        self.e12 = [([F(v) for v in x2[i]], F(o1[i, 0]), F(o1[i, 1]), F(s1[i])) for i in range(self.n)]
        self.e21 = [([F(v) for v in x1[i]], F(o2[i, 0]), F(o2[i, 1]), F(s2[i])) for i in range(self.n)]
        self.th2 = F(f32(th2)); self.delta = F(f32(np.sqrt(F(f32(th2))))); self.fix = bool(fix_scale)
        self.removed = [False] * self.n

    def sums(self, est, full):
        TT = [perturbed(est, k, self.fix) for k in range(15 if full else 1)]
        T = [t[0] for t in TT]; Ti = [t[1] for t in TT]
        S = [ZERO] * 36
        for i in range(self.n):
            if self.removed[i]:
                continue
            for c in (edge_contrib(T, self.K1, self.e12[i], self.delta, full), edge_contrib(Ti, self.K2, self.e21[i], self.delta, full)):
                if full:
                    for k in range(35):
                        S[k] = S[k] + c[k]
                S[35] = S[35] + c[35]
        return S

    def classify(self, Serr):
        """-> (nBad, nIn)"""
        Sinv = inverse(Serr)
        nBad = nIn = 0
        for i in range(self.n):
            if self.removed[i]:
                continue
            c12 = edge_error(Serr, self.K1, *self.e12[i])[0]; c21 = edge_error(Sinv, self.K2, *self.e21[i])[0]
            if bool(c12 > self.th2) or bool(c21 > self.th2):
                self.removed[i] = True; nBad += 1
            else:
                nIn += 1
        return nBad, nIn


def optimize_sim3(item, th2=10.0, fix_scale=True, trace=None):
    """item: the dict of ORBmatcher.OptimizeSim3.  -> dict of the outputs of sind_sim3opt_item.  trace: a list that gets (stage, iteration, iniChi) per linearisation and
    (stage, iteration, 'trial', tempChi, accepted) per trial, (stage, 'classified', removed after it) per stage"""
    with np.errstate(all="ignore"):
        return _optimize_sim3(item, th2, fix_scale, trace)


def _optimize_sim3(item, th2, fix_scale, trace):
    g = Graph(item, th2, fix_scale)
    n = g.n
    S0 = from_input(item["s12"], item["R12"], item["t12"])
    out = dict(q=np.array(S0[0]), t=np.array(S0[1]), s=S0[2], removed=np.zeros(n, np.uint8), n_inliers=0, n_bad=0, n_stages=0, stage_iters=np.zeros(2, np.int32), stage_chi2=np.zeros(2),
               stage_lambda=np.zeros(2))
    if n < 1:
        return out
    est = S0; errS = S0
    x = [ZERO] * 7
    lam, ni = F(-1.0), F(2.0)
    nBad = nIn = 0
    for stage in range(2):
        iterations = 5 if stage == 0 else (10 if nBad > 0 else 5)
        cj, nBadLM, ok, currentChi = 0, 0, True, ZERO
        i = 0
        while i < iterations and ok:
            S = g.sums(est, True); errS = est
            currentChi = S[35]; tempChi = currentChi; iniChi = currentChi
            if trace is not None:
                trace.append((stage, i, iniChi))
            H = [[ZERO] * 7 for _ in range(7)]; k = 0
            for a in range(7):
                for c in range(a, 7):
                    H[a][c] = S[k]; H[c][a] = S[k]; k += 1
            b = S[28:35]
            if i == 0:
                maxDiagonal = ZERO
                for j in range(7):
                    a = abs(H[j][j]); maxDiagonal = maxDiagonal if a < maxDiagonal else a
                lam = F(1e-5) * maxDiagonal; ni = F(2.0); nBadLM = 0
            rho = ZERO; qmax = 0
            while True:
                backup = est
                Hl = [[H[a][c] + lam if a == c else H[a][c] for c in range(7)] for a in range(7)]
                ok2, x = ldlt_solve(Hl, b, x)
                est, x = oplus(x, g.fix, est)
                T = g.sums(est, False); errS = est
                tempChi = T[35]
                if not ok2:
                    tempChi = DBL_MAX
                rho = currentChi - tempChi
                scale = ZERO
                for j in range(7):
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
                    trace.append((stage, i, "trial", tempChi, good))
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
        out["stage_iters"][stage] = cj; out["stage_chi2"][stage] = currentChi; out["stage_lambda"][stage] = lam; out["n_stages"] = stage + 1
        bad, nIn = g.classify(errS)
        out["removed"] = np.array(g.removed, np.uint8)
        if trace is not None:
            trace.append((stage, "classified", list(g.removed)))
        if stage == 0:
            nBad = bad; out["n_bad"] = nBad
            if n - nBad < 10:
                return out
    out["q"] = np.array(est[0]); out["t"] = np.array(est[1]); out["s"] = est[2]; out["n_inliers"] = nIn
    return out
