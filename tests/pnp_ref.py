"""Sequential restatement of the reference's PnPsolver (src/PnPsolver.cc) for the tests: EPnP (compute_pose and what it calls, :375-950), CheckInliers (:308-339),
SetRansacParameters (:121-157), Refine (:260-305), the literal iterate (:165-258, with its or-condition) and the loop of Tracking::Relocalization
(src/Tracking.cc:1435-1527).  It shares no code with csrc/host/epnp.hpp: scalars only (Python floats are IEEE FP64, np.float32 where the reference has a float),
every sum an explicit sequential loop (np.sum adds pairwise).  The OpenCV 4.2.0 primitives are restated as that header lists them; parity with a real OpenCV is unpinned."""
from __future__ import annotations

import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
NAN = float("nan")
F = np.float32


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if x >= 0 or x != x else NAN


def _log(x):
    return math.log(x) if x > 0 else -math.inf if x == 0 else NAN


def cv_hypot(a, b):
    a = abs(a); b = abs(b)
    if a > b:
        b = _div(b, a); return a * _sqrt(1 + b * b)
    if b > 0:
        a = _div(a, b); return b * _sqrt(1 + a * a)
    return 0.0


def jacobi_svd(At, m, n, n1, want_v=True):
    """JacobiSVDImpl_<double>: At = list of n rows of m; -> W [n], Vt (n rows of n, or None); At is rotated in place"""
    eps = DBL_EPSILON * 10
    W = [0.0] * n
    Vt = [[1.0 if i == k else 0.0 for k in range(n)] for i in range(n)] if want_v else None
    for i in range(n):
        sd = 0.0
        for k in range(m):
            t = At[i][k]; sd += t * t
        W[i] = sd
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, p, b = W[i], 0.0, W[j]
                for k in range(m):
                    p += Ai[k] * Aj[k]
                if abs(p) <= eps * _sqrt(a * b):
                    continue
                p *= 2
                beta = a - b; gamma = cv_hypot(p, beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = _sqrt(_div(delta, gamma)); c = _div(p, gamma * s * 2)
                else:
                    c = _sqrt(_div(gamma + beta, gamma * 2)); s = _div(p, gamma * c * 2)
                a = b = 0.0
                for k in range(m):
                    t0 = c * Ai[k] + s * Aj[k]; t1 = -s * Ai[k] + c * Aj[k]
                    Ai[k] = t0; Aj[k] = t1
                    a += t0 * t0; b += t1 * t1
                W[i] = a; W[j] = b
                changed = True
                if want_v:
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(n):
                        t0 = c * Vi[k] + s * Vj[k]; t1 = -s * Vi[k] + c * Vj[k]
                        Vi[k] = t0; Vj[k] = t1
        if not changed:
            break
    for i in range(n):
        sd = 0.0
        for k in range(m):
            t = At[i][k]; sd += t * t
        W[i] = _sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            if want_v:
                Vt[i], Vt[j] = Vt[j], Vt[i]
    Wout = list(W)
    state = 0x12345678
    for i in range(n1):
        sd = W[i] if i < n else 0.0
        ii = 0
        while ii < 100 and sd <= DBL_MIN:
            val0 = 1.0 / m
            for k in range(m):
                state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
                At[i][k] = val0 if (state & 0xFFFFFFFF) & 256 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = 0.0
                    for k in range(m):
                        sd += At[i][k] * At[j][k]
                    asum = 0.0
                    for k in range(m):
                        t = At[i][k] - sd * At[j][k]; At[i][k] = t; asum += abs(t)
                    asum = _div(1, asum) if asum > eps * 100 else 0.0
                    for k in range(m):
                        At[i][k] *= asum
                sd = 0.0
                for k in range(m):
                    t = At[i][k]; sd += t * t
                sd = _sqrt(sd)
            ii += 1
        s = _div(1, sd) if sd > DBL_MIN else 0.0
        for k in range(m):
            At[i][k] *= s
    return Wout, Vt


def solve_svd(A, nc, b):
    """cvSolve(A [6][nc], b, x, CV_SVD)"""
    At = [[A[k][i] for k in range(6)] for i in range(nc)]
    W, Vt = jacobi_svd(At, 6, nc, nc)
    x = [0.0] * nc
    threshold = 0.0
    for i in range(nc):
        threshold += W[i]
    threshold *= DBL_EPSILON * 2
    for i in range(nc):
        wi = W[i]
        if abs(wi) <= threshold:
            continue
        wi = _div(1, wi)
        s = 0.0
        for j in range(6):
            s += At[i][j] * b[j]
        s *= wi
        for j in range(nc):
            x[j] = x[j] + s * Vt[i][j]
    return x


def invert3(A):
    At = [[A[k][i] for k in range(3)] for i in range(3)]
    W, Vt = jacobi_svd(At, 3, 3, 3)
    X = [[0.0] * 3 for _ in range(3)]
    threshold = 0.0
    for i in range(3):
        threshold += W[i]
    threshold *= DBL_EPSILON * 2
    for i in range(3):
        wi = W[i]
        if abs(wi) <= threshold:
            continue
        wi = _div(1, wi)
        buf = [At[i][j] * wi for j in range(3)]
        for r in range(3):
            for j in range(3):
                X[r][j] = X[r][j] + Vt[i][r] * buf[j]
    return X


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def dist2(p, q):
    return (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2])


def qr_solve(A, b, X):
    """A: flat 24 (6 x 4), b: 6, X: 4; all modified in place; X untouched when A is singular"""
    nr, nc = 6, 4
    A1 = [0.0] * nr; A2 = [0.0] * nr
    kk = 0
    for k in range(nc):
        ik = kk; eta = abs(A[ik])
        for i in range(k + 1, nr):
            elt = abs(A[ik])
            if eta < elt:
                eta = elt
            ik += nc
        if eta == 0:
            return
        ik = kk; sm = 0.0; inv_eta = _div(1.0, eta)
        for i in range(k, nr):
            A[ik] *= inv_eta; sm += A[ik] * A[ik]; ik += nc
        sigma = _sqrt(sm)
        if A[kk] < 0:
            sigma = -sigma
        A[kk] += sigma
        A1[k] = sigma * A[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            ik = kk; sm = 0.0
            for i in range(k, nr):
                sm += A[ik] * A[ik + j - k]; ik += nc
            tau = _div(sm, A1[k])
            ik = kk
            for i in range(k, nr):
                A[ik + j - k] -= tau * A[ik]; ik += nc
        kk += nc + 1
    jj = 0
    for j in range(nc):
        ij = jj; tau = 0.0
        for i in range(j, nr):
            tau += A[ij] * b[i]; ij += nc
        tau = _div(tau, A1[j])
        ij = jj
        for i in range(j, nr):
            b[i] -= tau * A[ij]; ij += nc
        jj += nc + 1
    X[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        ij = i * nc + i + 1; sm = 0.0
        for j in range(i + 1, nc):
            sm += A[ij] * X[j]; ij += 1
        X[i] = _div(b[i] - sm, A2[i])


def gauss_newton(L, rho, betas):
    x = [0.0] * 4                                                       # uninitialised in the reference; defined as zeros (csrc/host/epnp.hpp)
    for _ in range(5):
        A = [0.0] * 24; b = [0.0] * 6
        for i in range(6):
            r = L[i]; B = betas
            A[4 * i] = 2 * r[0] * B[0] + r[1] * B[1] + r[3] * B[2] + r[6] * B[3]
            A[4 * i + 1] = r[1] * B[0] + 2 * r[2] * B[1] + r[4] * B[2] + r[7] * B[3]
            A[4 * i + 2] = r[3] * B[0] + r[4] * B[1] + 2 * r[5] * B[2] + r[8] * B[3]
            A[4 * i + 3] = r[6] * B[0] + r[7] * B[1] + r[8] * B[2] + 2 * r[9] * B[3]
            b[i] = rho[i] - (r[0] * B[0] * B[0] + r[1] * B[0] * B[1] + r[2] * B[1] * B[1] + r[3] * B[0] * B[2] + r[4] * B[1] * B[2] + r[5] * B[2] * B[2] +
                             r[6] * B[0] * B[3] + r[7] * B[1] * B[3] + r[8] * B[2] * B[3] + r[9] * B[3] * B[3])
        qr_solve(A, b, x)
        for i in range(4):
            betas[i] += x[i]


def find_betas(which, L, rho):
    cols = {1: [0, 1, 3, 6], 2: [0, 1, 2], 3: [0, 1, 2, 3, 4]}[which]
    b = solve_svd([[L[i][c] for c in cols] for i in range(6)], len(cols), rho)
    be = [0.0] * 4
    if which == 1:
        if b[0] < 0:
            be[0] = _sqrt(-b[0]); be[1] = _div(-b[1], be[0]); be[2] = _div(-b[2], be[0]); be[3] = _div(-b[3], be[0])
        else:
            be[0] = _sqrt(b[0]); be[1] = _div(b[1], be[0]); be[2] = _div(b[2], be[0]); be[3] = _div(b[3], be[0])
        return be
    if b[0] < 0:
        be[0] = _sqrt(-b[0]); be[1] = _sqrt(-b[2]) if b[2] < 0 else 0.0
    else:
        be[0] = _sqrt(b[0]); be[1] = _sqrt(b[2]) if b[2] > 0 else 0.0
    if b[1] < 0:
        be[0] = -be[0]
    be[2] = 0.0 if which == 2 else _div(b[3], be[0])
    return be


def svd3_uv(A):
    """cvSVD(A, D, U, V, CV_SVD_MODIFY_A) of a 3 x 3 -> U, V with singular vectors in their columns"""
    At = [[A[k][i] for k in range(3)] for i in range(3)]
    _, Vt = jacobi_svd(At, 3, 3, 3)
    return [[At[k][i] for k in range(3)] for i in range(3)], [[Vt[k][i] for k in range(3)] for i in range(3)]


def compute_pose(pws, us, fu, fv, uc, vc):
    """pws [n][3], us [n][2] (any floats; widened to FP64 as add_correspondence does) -> R (3 lists), t, reprojection error"""
    pws = [[float(v) for v in p] for p in pws]; us = [[float(v) for v in u] for u in us]
    n = len(pws)
    # choose_control_points
    cws = [[0.0] * 3 for _ in range(4)]
    for i in range(n):
        for j in range(3):
            cws[0][j] += pws[i][j]
    for j in range(3):
        cws[0][j] = _div(cws[0][j], n)
    P = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            s = 0.0
            for k in range(n):
                s += (pws[k][i] - cws[0][i]) * (pws[k][j] - cws[0][j])
            P[i][j] = s * 1.0; P[j][i] = P[i][j]
    dc, _ = jacobi_svd(P, 3, 3, 3, want_v=False)
    for i in range(1, 4):
        k = _sqrt(_div(dc[i - 1], n))
        for j in range(3):
            cws[i][j] = cws[0][j] + k * P[i - 1][j]
    # compute_barycentric_coordinates
    cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
    ci = invert3(cc)
    alphas = []
    for i in range(n):
        p = pws[i]; a = [0.0] * 4
        for j in range(3):
            a[1 + j] = ci[j][0] * (p[0] - cws[0][0]) + ci[j][1] * (p[1] - cws[0][1]) + ci[j][2] * (p[2] - cws[0][2])
        a[0] = 1.0 - a[1] - a[2] - a[3]
        alphas.append(a)
    # fill_M
    M = []
    for i in range(n):
        a = alphas[i]; u, v = us[i]
        r1 = []; r2 = []
        for c in range(4):
            r1 += [a[c] * fu, 0.0, a[c] * (uc - u)]
            r2 += [0.0, a[c] * fv, a[c] * (vc - v)]
        M.append(r1); M.append(r2)
    # cvMulTransposed + cvSVD
    mtm = [[0.0] * 12 for _ in range(12)]
    for i in range(12):
        for j in range(i, 12):
            s = 0.0
            for k in range(2 * n):
                s += M[k][i] * M[k][j]
            mtm[i][j] = s * 1.0; mtm[j][i] = mtm[i][j]
    jacobi_svd(mtm, 12, 12, 12, want_v=False)
    ut = mtm
    # compute_L_6x10, compute_rho
    v = [ut[11], ut[10], ut[9], ut[8]]
    dv = [[None] * 6 for _ in range(4)]
    for i in range(4):
        a, b = 0, 1
        for j in range(6):
            dv[i][j] = [v[i][3 * a] - v[i][3 * b], v[i][3 * a + 1] - v[i][3 * b + 1], v[i][3 * a + 2] - v[i][3 * b + 2]]
            b += 1
            if b > 3:
                a += 1; b = a + 1
    L = []
    for i in range(6):
        L.append([dot3(dv[0][i], dv[0][i]), 2.0 * dot3(dv[0][i], dv[1][i]), dot3(dv[1][i], dv[1][i]), 2.0 * dot3(dv[0][i], dv[2][i]), 2.0 * dot3(dv[1][i], dv[2][i]),
                  dot3(dv[2][i], dv[2][i]), 2.0 * dot3(dv[0][i], dv[3][i]), 2.0 * dot3(dv[1][i], dv[3][i]), 2.0 * dot3(dv[2][i], dv[3][i]), dot3(dv[3][i], dv[3][i])])
    rho = [dist2(cws[0], cws[1]), dist2(cws[0], cws[2]), dist2(cws[0], cws[3]), dist2(cws[1], cws[2]), dist2(cws[1], cws[3]), dist2(cws[2], cws[3])]

    def R_and_t(betas):
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            vv = ut[11 - i]
            for j in range(4):
                for k in range(3):
                    ccs[j][k] += betas[i] * vv[3 * j + k]
        pcs = []
        for i in range(n):
            a = alphas[i]
            pcs.append([a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j] for j in range(3)])
        if pcs[0][2] < 0.0:
            pcs = [[-c for c in pc] for pc in pcs]
        pc0 = [0.0] * 3; pw0 = [0.0] * 3
        for i in range(n):
            for j in range(3):
                pc0[j] += pcs[i][j]; pw0[j] += pws[i][j]
        for j in range(3):
            pc0[j] = _div(pc0[j], n); pw0[j] = _div(pw0[j], n)
        abt = [[0.0] * 3 for _ in range(3)]
        for i in range(n):
            for j in range(3):
                for k in range(3):
                    abt[j][k] += (pcs[i][j] - pc0[j]) * (pws[i][k] - pw0[k])
        U, V = svd3_uv(abt)
        R = [[dot3(U[i], V[j]) for j in range(3)] for i in range(3)]
        det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
               R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
        if det < 0:
            R[2] = [-R[2][0], -R[2][1], -R[2][2]]
        t = [pc0[0] - dot3(R[0], pw0), pc0[1] - dot3(R[1], pw0), pc0[2] - dot3(R[2], pw0)]
        sum2 = 0.0
        for i in range(n):
            pw = pws[i]
            Xc = dot3(R[0], pw) + t[0]; Yc = dot3(R[1], pw) + t[1]; inv_Zc = _div(1.0, dot3(R[2], pw) + t[2])
            ue = uc + fu * Xc * inv_Zc; ve = vc + fv * Yc * inv_Zc
            u, vv = us[i]
            sum2 += _sqrt((u - ue) * (u - ue) + (vv - ve) * (vv - ve))
        return R, t, _div(sum2, n)

    res = [None] * 4
    for w in (1, 2, 3):
        be = find_betas(w, L, rho)
        gauss_newton(L, rho, be)
        res[w] = R_and_t(be)
    N = 1
    if res[2][2] < res[1][2]:
        N = 2
    if res[3][2] < res[N][2]:
        N = 3
    return res[N]


def check_inliers(x3Dw, p2d, sigma2, th2, fu, fv, uc, vc, R, t):
    """CheckInliers -> (mvbInliersi bool [n], mnInliersi)"""
    n = len(sigma2); inl = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            X, Y, Z = (float(v) for v in x3Dw[i])
            Xc = F(R[0][0] * X + R[0][1] * Y + R[0][2] * Z + t[0])
            Yc = F(R[1][0] * X + R[1][1] * Y + R[1][2] * Z + t[1])
            invZc = F(_div(1, R[2][0] * X + R[2][1] * Y + R[2][2] * Z + t[2]))
            ue = uc + fu * float(Xc) * float(invZc); ve = vc + fv * float(Yc) * float(invZc)
            distX = F(float(p2d[i][0]) - ue); distY = F(float(p2d[i][1]) - ve)
            error2 = F(F(distX * distX) + F(distY * distY))
            inl[i] = bool(error2 < F(F(sigma2[i]) * F(th2)))
    return inl, int(inl.sum())


def ransac_params(n, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4):
    """SetRansacParameters -> (mRansacMinInliers, mRansacMaxIts)"""
    eps = F(epsilon)
    nMin = int(F(n) * eps)                                              # int * float: the int is converted to float
    nMin = max(nMin, minInliers, minSet)
    with np.errstate(all="ignore"):
        if eps < F(nMin) / F(n):
            eps = F(nMin) / F(n)
    if nMin == n:
        its = 1
    else:
        q = _div(_log(1 - probability), _log(1 - math.pow(float(eps), 3)))
        # the reference converts ceil(q) to int unbounded, which is undefined for a NaN or an infinity; the library bounds first, a NaN to maxIterations (csrc/host/pnp.cpp)
        its = maxIterations if q != q or q == math.inf else 1 if q == -math.inf else math.ceil(q)
    return nMin, max(1, min(its, maxIterations))


def refine_plan(counts, min_inliers, best_count, has_best):
    """-> (refine_of_hyp, hyp_of_refine): the distinct Refine problems, see csrc/host/pnp.hpp"""
    best, cur, of_hyp, hyps = best_count, -1, [], []
    for h, c in enumerate(counts):
        if c < min_inliers:
            of_hyp.append(-1); continue
        if c > best:
            best = c; cur = len(hyps); hyps.append(h)
        elif cur < 0:
            if not has_best:
                of_hyp.append(-2); continue
            cur = len(hyps); hyps.append(-1)
        of_hyp.append(cur)
    return of_hyp, hyps


def pack_bits(inl):
    n = len(inl); w = np.zeros((n + 63) // 64, np.uint64)
    for i in np.flatnonzero(inl):
        w[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return w


def unpack_bits(w, n):
    i = np.arange(n)
    return ((np.asarray(w, np.uint64)[i >> 6] >> (i & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


class Evaluator:
    """What sind_match_pnp_ransac computes, by this module, for sindslam_amd.pnp.PnPsolver(evaluate=...).  Poses and refines are kept per (candidate, sample) and
    per (candidate, inlier set), so a schedule that is drawn again costs nothing twice.  A candidate is known by inp["key"] (pnp_scene.candidate sets it)."""

    def __init__(self, K):
        self.K = tuple(float(F(k)) for k in K); self.poses = {}; self.refines = {}; self.calls = 0

    def hyp(self, inp, sample):
        key = (inp["key"], tuple(int(s) for s in sample))
        if key not in self.poses:
            R, t, _ = compute_pose([inp["x3Dw"][i] for i in key[1]], [inp["p2d"][i] for i in key[1]], *self.K)
            inl, cnt = check_inliers(inp["x3Dw"], inp["p2d"], inp["sigma2"], inp["th2"], *self.K, R, t)
            self.poses[key] = (R, t, inl, cnt)
        return self.poses[key]

    def refine(self, inp, inl):
        key = (inp["key"], inl.tobytes())
        if key not in self.refines:
            idx = np.flatnonzero(inl)
            R, t, _ = compute_pose([inp["x3Dw"][i] for i in idx], [inp["p2d"][i] for i in idx], *self.K)
            rin, cnt = check_inliers(inp["x3Dw"], inp["p2d"], inp["sigma2"], inp["th2"], *self.K, R, t)
            self.refines[key] = (R, t, rin, cnt)
        return self.refines[key]

    def __call__(self, requests):
        self.calls += 1
        out = []
        for inp, samples, min_inliers, best_count, best_bits in requests:
            n = len(inp["sigma2"])
            hs = [self.hyp(inp, s) for s in samples]
            of_hyp, hyps = refine_plan([h[3] for h in hs], min_inliers, best_count, best_bits is not None)
            rs = [self.refine(inp, unpack_bits(best_bits, n) if h < 0 else hs[h][2]) for h in hyps]
            out.append(dict(count=np.array([h[3] for h in hs], np.int32), bits=np.array([pack_bits(h[2]) for h in hs], np.uint64).reshape(len(hs), (n + 63) // 64),
                            R=np.array([h[0] for h in hs], np.float64).reshape(-1, 3, 3), t=np.array([h[1] for h in hs], np.float64).reshape(-1, 3),
                            refine=np.array(of_hyp, np.int32), refine_hyp=np.array(hyps, np.int32), refine_count=np.array([r[3] for r in rs], np.int32),
                            refine_bits=np.array([pack_bits(r[2]) for r in rs], np.uint64).reshape(len(rs), (n + 63) // 64),
                            refine_R=np.array([r[0] for r in rs], np.float64).reshape(-1, 3, 3), refine_t=np.array([r[1] for r in rs], np.float64).reshape(-1, 3)))
        return out


def random_int(raw, lo, hi, rand_max=2147483647):
    """DUtils::Random::RandomInt on a raw rand() value"""
    d = hi - lo + 1
    return int((float(raw) / (float(rand_max) + 1.0)) * d) + lo


class LiteralPnPsolver:
    """PnPsolver as written: draws from `rand` when the reference does, evaluates at once.  inp: x3Dw, p2d, sigma2, indices (mvKeyPointIndices), n_keypoints"""

    def __init__(self, ev, inp, rand, counter):
        self.ev, self.inp, self.rand, self.counter = ev, inp, rand, counter
        self.N = len(inp["sigma2"]); self.mnIterations = 0; self.mnBestInliers = 0; self.mvbBestInliers = None; self.mBestTcw = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        self.mRansacMinInliers, self.mRansacMaxIts = ransac_params(self.N, probability, minInliers, maxIterations, minSet, epsilon)
        self.mRansacMinSet = minSet; self.inp["th2"] = float(F(th2))

    @staticmethod
    def tcw(R, t):
        T = np.eye(4, dtype=np.float32); T[:3, :3] = np.array(R, np.float64).astype(np.float32); T[:3, 3] = np.array(t, np.float64).astype(np.float32)
        return T

    def out(self, inl):
        vb = np.zeros(self.inp["n_keypoints"], bool); vb[np.asarray(self.inp["indices"])[inl]] = True
        return vb

    def iterate(self, nIterations):
        if self.N < self.mRansacMinInliers:
            return None, True, np.zeros(0, bool), 0
        nCur = 0
        while self.mnIterations < self.mRansacMaxIts or nCur < nIterations:
            nCur += 1; self.mnIterations += 1
            avail = list(range(self.N)); sample = []
            for _ in range(self.mRansacMinSet):
                self.counter[0] += 1
                randi = random_int(self.rand(), 0, len(avail) - 1)
                sample.append(avail[randi]); avail[randi] = avail[-1]; avail.pop()
            R, t, inl, cnt = self.ev.hyp(self.inp, sample)
            if cnt >= self.mRansacMinInliers:
                if cnt > self.mnBestInliers:
                    self.mvbBestInliers = inl.copy(); self.mnBestInliers = cnt; self.mBestTcw = self.tcw(R, t)
                rR, rt, rin, rcnt = self.ev.refine(self.inp, self.mvbBestInliers)                # Refine()
                if rcnt > self.mRansacMinInliers:
                    return self.tcw(rR, rt), False, self.out(rin), rcnt
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                return self.mBestTcw.copy(), True, self.out(self.mvbBestInliers), self.mnBestInliers
            return None, True, np.zeros(0, bool), 0
        return None, False, np.zeros(0, bool), 0


def literal_relocalization(solvers, accept, trace=None):
    """Tracking.cc:1435-1527 -> (index of the accepted candidate or -1, Tcw, vbInliers, vbDiscarded, the order in which candidates were discarded)"""
    discarded = [s is None for s in solvers]; order = []
    nCandidates = sum(not d for d in discarded)
    while nCandidates > 0:
        for i, s in enumerate(solvers):
            if discarded[i]:
                continue
            Tcw, bNoMore, vb, nInl = s.iterate(5)
            if trace is not None:
                trace.append((i, bool(bNoMore)))
            if bNoMore:
                discarded[i] = True; nCandidates -= 1; order.append(i)
            if Tcw is not None and accept(i, Tcw, vb, nInl):
                return i, Tcw, vb, discarded, order
    return -1, None, None, discarded, order
