"""Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:781-1044) restated in Python with NumPy FP64 scalars, operation for operation as
sindslam_amd/csrc/host/essential_graph.hpp has it: the defined log and acos, Sim3::log with its four branches and the 3 x 3 partial-pivot LU, the numeric Jacobians of
EdgeSim3 on both vertices, the ordered sums, the Levenberg-Marquardt loop with the user's initial lambda, the recovery of poses and points.  The linear solve here is
the DENSE natural-order LDL^T of the definition, not the envelope: that the envelope gives the same bits is what tests/test_essgraph_cpu.py checks with it.  Sim3's
exponential, product, inverse and map are sim3opt_ref's, the quaternion helpers and sincos poseopt_ref's (as the header takes them from sim3_opt.hpp and pose_opt.hpp).
Bit equality with the host library is BY CONSTRUCTION of the two texts; the test asserts it and checks the result against things that are neither."""
from __future__ import annotations

import math

import numpy as np

import sim3opt_ref as SR
from poseopt_ref import DBL_MAX, F, HALF, ONE, TWO, ZERO, f32, quat_to_matrix, sincos

TWO20 = F(1048576.0)
DELTA = F(1e-9)


def log(x):
    x = F(x)
    ln2_hi, ln2_lo = F(6.93147180369123816490e-01), F(1.90821492927058770002e-10)
    Lg1, Lg2, Lg3, Lg4, Lg5, Lg6, Lg7 = (F(v) for v in (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
                                                        1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01))
    if not (x == x):
        return x
    if x < 0.0:
        return F(np.nan)
    if x == 0.0:
        return F(-np.inf)
    if x > DBL_MAX:
        return x
    m, ex = math.frexp(float(x))
    xn = F(m) * TWO; k = ex - 1
    halved = bool(xn >= ONE + F(434332.0) / TWO20)
    if halved:
        xn = xn * HALF; k = k + 1
    f = xn - ONE; dk = F(k)
    if f >= -ONE / TWO20 and f < ONE / TWO20:
        if f == 0.0:
            return ZERO if k == 0 else dk * ln2_hi + dk * ln2_lo
        R = f * f * (HALF - F(0.33333333333333333) * f)
        return f - R if k == 0 else dk * ln2_hi - ((R - dk * ln2_lo) - f)
    s = f / (TWO + f); z = s * s; w = z * z
    t1 = w * (Lg2 + w * (Lg4 + w * Lg6)); t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)))
    R = t2 + t1
    mid = bool(xn < (ONE + F(440402.0) / TWO20) * HALF) if halved else bool(xn >= ONE + F(398458.0) / TWO20)
    if mid:
        hfsq = HALF * f * f
        return f - (hfsq - s * (hfsq + R)) if k == 0 else dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)
    return f - s * (f - R) if k == 0 else dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f)


def acos(x):
    x = F(x)
    pio2_hi, pio2_lo, pi = F(1.57079632679489655800e+00), F(6.12323399573676603587e-17), F(3.14159265358979311600e+00)
    pS0, pS1, pS2, pS3, pS4, pS5 = (F(v) for v in (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
                                                   7.91534994289814532176e-04, 3.47933107596021167570e-05))
    qS1, qS2, qS3, qS4 = (F(v) for v in (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02))
    P = lambda z: z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))))
    Q = lambda z: ONE + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)))
    if not (x == x):
        return x
    ax = abs(x)
    if ax >= 1.0:
        if ax == 1.0:
            return ZERO if x > 0.0 else pi + TWO * pio2_lo
        return F(np.nan)
    if ax < 0.5:
        if ax <= F(6.938893903907228e-18):
            return pio2_hi + pio2_lo
        z = x * x
        r = P(z) / Q(z)
        return pio2_hi - (x - (pio2_lo - r * x))
    if x < 0.0:
        z = (ONE + x) * HALF
        p = P(z); q = Q(z)
        s = np.sqrt(z); r = p / q; w = r * s - pio2_lo
        return pi - TWO * (s + w)
    z = (ONE - x) * HALF; s = np.sqrt(z)
    sp = s * F(134217729.0); df = sp - (sp - s)
    c = (z - df * df) / (s + df)
    r = P(z) / Q(z); w = r * s + c
    return TWO * (df + w)


def lu3_solve(W, t):
    a = [list(r) for r in W]; b = list(t)
    for c in range(2):
        piv = c; best = abs(a[c][c])
        for r in range(c + 1, 3):
            if abs(a[r][c]) > best:
                best = abs(a[r][c]); piv = r
        if piv != c:
            a[c], a[piv] = a[piv], a[c]; b[c], b[piv] = b[piv], b[c]
        for r in range(c + 1, 3):
            f = a[r][c] / a[c][c]
            for k in range(c + 1, 3):
                a[r][k] = a[r][k] - f * a[c][k]
            b[r] = b[r] - f * b[c]
    u = [ZERO] * 3
    u[2] = b[2] / a[2][2]
    u[1] = (b[1] - a[1][2] * u[2]) / a[1][1]
    u[0] = ((b[0] - a[0][1] * u[1]) - a[0][2] * u[2]) / a[0][0]
    return u


def sim3_log(S):
    q, t, s = S
    sigma = log(s)
    R = quat_to_matrix(q)
    d = HALF * (R[0][0] + R[1][1] + R[2][2] - ONE)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    eps = F(0.00001)
    near = bool(d > ONE - eps)
    theta, sn, cs = ZERO, ZERO, ONE
    if near:
        om = [HALF * v for v in dR]
    else:
        theta = acos(d)
        f = theta / (TWO * np.sqrt(ONE - d * d))
        om = [f * v for v in dR]
        sn, cs = sincos(theta)
    if abs(sigma) < eps:
        C = ONE
        if near:
            A = ONE / TWO; B = ONE / F(6.0)
        else:
            theta2 = theta * theta
            A = (ONE - cs) / theta2; B = (theta - sn) / (theta2 * theta)
    else:
        C = (s - ONE) / sigma
        if near:
            sigma2 = sigma * sigma
            A = ((sigma - ONE) * s + ONE) / sigma2
            B = ((HALF * sigma2 - sigma + ONE) * s) / (sigma2 * sigma)
        else:
            theta2 = theta * theta; a = s * sn; b = s * cs; c = theta2 + sigma * sigma
            A = (a * sigma + (ONE - b) * theta) / (theta * c)
            B = (C - ((b - ONE) * sigma + a * theta) / c) * ONE / theta2
    O = [[ZERO, -om[2], om[1]], [om[2], ZERO, -om[0]], [-om[1], om[0], ZERO]]
    W = [[(A * O[i][j] + B * (O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j])) + C * (ONE if i == j else ZERO) for j in range(3)] for i in range(3)]
    up = lu3_solve(W, t)
    return [om[0], om[1], om[2], up[0], up[1], up[2], sigma]


def load8(p):
    return ([F(v) for v in p[0:4]], [F(v) for v in p[4:7]], F(p[7]))


def store8(S):
    return [*S[0], *S[1], S[2]]


def edge_error(C, Si, SjInv):
    return sim3_log(SR.mul(SR.mul(C, Si), SjInv))


def tri(r, c):
    return r * 7 - r * (r - 1) // 2 + (c - r)


def dense_ldlt_solve(H, b, lam):
    """the definition: H + lam I = L D L^T in natural order without pivoting; H full symmetric [n][n].  -> (ok, x); not ok: a zero pivot"""
    n = len(b)
    L = [[ZERO] * n for _ in range(n)]; D = [ZERO] * n
    for j in range(n):
        for i in range(j, n):
            v = H[j][i] + lam if i == j else H[j][i]
            for k in range(j):
                v = v - (L[i][k] * D[k]) * L[j][k]
            if i == j:
                D[j] = v
            else:
                L[i][j] = v / D[j]
    if any(d == 0.0 for d in D):
        return False, None
    y = list(b)
    for j in range(n):
        for i in range(j + 1, n):
            y[i] = y[i] - L[i][j] * y[j]
    y = [y[i] / D[i] for i in range(n)]
    for j in range(n - 1, 0, -1):
        for i in range(j):
            y[i] = y[i] - L[j][i] * y[j]
    return True, y


class Graph:
    def __init__(self, it, fix_scale):
        self.fix = bool(fix_scale)
        self.n_kf = len(it["kf_id"]); self.n_e = len(it["edge_i"])
        self.ei = [int(v) for v in it["edge_i"]]; self.ej = [int(v) for v in it["edge_j"]]
        Tcw = np.asarray(it["Tcw"], np.float32).reshape(self.n_kf, 4, 4)
        self.vScw = []
        for i in range(self.n_kf):
            if it["has_corrected"][i]:
                self.vScw.append(load8(np.asarray(it["corrected"], np.float64).reshape(-1, 8)[i]))
            else:
                self.vScw.append(SR.from_input(1.0, Tcw[i, :3, :3], Tcw[i, :3, 3]))
        self.est = list(self.vScw)
        self.meas = []
        nc = np.asarray(it["noncorrected"], np.float64).reshape(-1, 8)
        for e in range(self.n_e):
            i, j = self.ei[e], self.ej[e]
            Siw, Sjw = self.vScw[i], self.vScw[j]
            if it["edge_kind"][e] == 1:
                if it["has_noncorrected"][i]:
                    Siw = load8(nc[i])
                if it["has_noncorrected"][j]:
                    Sjw = load8(nc[j])
            self.meas.append(SR.mul(Sjw, SR.inverse(Siw)))
        deg = [0] * self.n_kf
        for e in range(self.n_e):
            deg[self.ei[e]] += 1; deg[self.ej[e]] += 1
        self.v_idx = [-1] * self.n_kf; self.idx_v = []
        for i in range(self.n_kf):
            if i != int(it["fixed_kf"]) and deg[i]:
                self.v_idx[i] = len(self.idx_v); self.idx_v.append(i)
        self.n_act = len(self.idx_v); self.n = 7 * self.n_act
        self.fails = 0

    def errors(self):
        """computeActiveErrors -> activeChi2 as one chain in edge order"""
        inv = [SR.inverse(S) for S in self.est]
        self.err = [edge_error(self.meas[e], self.est[self.ei[e]], inv[self.ej[e]]) for e in range(self.n_e)]
        chi = ZERO
        for e in range(self.n_e):
            c = ZERO
            for d in range(7):
                c = c + self.err[e][d] * self.err[e][d]
            chi = chi + c
        return chi

    def linearize(self):
        chi = self.errors()
        T = {v: [SR.perturbed(self.est[v], k, self.fix) for k in range(15)] for v in self.idx_v}
        base = [(S, SR.inverse(S)) for S in self.est]
        scalar = ONE / (TWO * DELTA)
        n = self.n
        self.H = [[ZERO] * n for _ in range(n)]; self.b = [ZERO] * n
        for e in range(self.n_e):                                     # every entry receives its edges in ascending edge order: that is the order of this loop
            i, j = self.ei[e], self.ej[e]; a, b = self.v_idx[i], self.v_idx[j]
            J = [None, None]
            for side, (v, act) in enumerate(((i, a), (j, b))):
                if act < 0:
                    continue
                Jm = [[ZERO] * 7 for _ in range(7)]
                for d in range(7):
                    if side == 0:
                        ep = edge_error(self.meas[e], T[v][1 + 2 * d][0], base[j][1]); em = edge_error(self.meas[e], T[v][2 + 2 * d][0], base[j][1])
                    else:
                        ep = edge_error(self.meas[e], base[i][0], T[v][1 + 2 * d][1]); em = edge_error(self.meas[e], base[i][0], T[v][2 + 2 * d][1])
                    for row in range(7):
                        Jm[row][d] = scalar * (ep[row] - em[row])
                J[side] = Jm
            er = self.err[e]
            for side, act in ((0, a), (1, b)):
                if act < 0:
                    continue
                Jm = J[side]
                for r in range(7):
                    for c in range(r, 7):
                        h = ZERO
                        for d in range(7):
                            h = h + Jm[d][r] * Jm[d][c]
                        self.H[7 * act + r][7 * act + c] = self.H[7 * act + r][7 * act + c] + h
                        if c != r:
                            self.H[7 * act + c][7 * act + r] = self.H[7 * act + r][7 * act + c]
                    t = ZERO
                    for d in range(7):
                        t = t + Jm[d][r] * -er[d]
                    self.b[7 * act + r] = self.b[7 * act + r] + t
            if a >= 0 and b >= 0:
                for r in range(7):
                    for c in range(7):
                        h = ZERO
                        for d in range(7):
                            h = h + J[0][d][r] * J[1][d][c]
                        self.H[7 * a + r][7 * b + c] = self.H[7 * a + r][7 * b + c] + h
                        self.H[7 * b + c][7 * a + r] = self.H[7 * a + r][7 * b + c]
        return chi

    def solve(self, lam):
        ok, y = dense_ldlt_solve(self.H, self.b, lam)
        if ok:
            self.x = y
        else:
            self.fails += 1
        return ok

    def update(self):
        for a, v in enumerate(self.idx_v):
            self.est[v], u = SR.oplus(self.x[7 * a:7 * a + 7], self.fix, self.est[v])
            self.x[7 * a:7 * a + 7] = u

    def scale(self, lam):
        sc = ZERO
        for i in range(self.n):
            sc = sc + self.x[i] * (lam * self.x[i] + self.b[i])
        return sc

    def optimize(self, iterations, user_lambda):
        self.x = [ZERO] * self.n
        lam, ni, current, cj, n_bad, ok = F(-1.0), F(2.0), ZERO, 0, 0, True
        i = 0
        while i < iterations and ok:
            current = self.linearize(); temp = current; ini = current
            if i == 0:
                lam = F(user_lambda); ni = F(2.0); n_bad = 0
            rho, qmax = ZERO, 0
            while True:
                backup = list(self.est)
                ok2 = self.solve(lam)
                self.update()
                temp = self.errors()
                if not ok2:
                    temp = DBL_MAX
                rho = current - temp
                sc = self.scale(lam) + F(1e-3)
                rho = rho / sc
                if rho > 0 and np.abs(temp) <= DBL_MAX:
                    t = F(2.0) * rho - ONE
                    alpha = ONE - t * t * t
                    alpha = F(2.0) / F(3.0) if F(2.0) / F(3.0) < alpha else alpha
                    factor = alpha if ONE / F(3.0) < alpha else ONE / F(3.0)
                    lam = lam * factor; ni = F(2.0); current = temp
                else:
                    lam = lam * ni; ni = ni * F(2.0); self.est = backup
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            terminate = False
            if qmax == 10 or rho == 0:
                terminate = True
            else:
                n_bad = n_bad + 1 if (ini - current) * F(1e3) < ini else 0
                if n_bad >= 3:
                    terminate = True
            ok = not terminate; cj += 1; i += 1
        return cj, current, lam


def recover(g, it):
    """:999-1040 -> Siw, Tiw, x3Dw"""
    Siw = np.array([store8(S) for S in g.est], np.float64).reshape(g.n_kf, 8)
    Tiw = np.zeros((g.n_kf, 4, 4), np.float32)
    Swc = []
    for i, S in enumerate(g.est):
        Swc.append(SR.inverse(S))
        R = quat_to_matrix(S[0]); f = ONE / S[2]
        for r in range(3):
            for c in range(3):
                Tiw[i, r, c] = f32(R[r][c])
            Tiw[i, r, 3] = f32(S[1][r] * f)
        Tiw[i, 3, 3] = 1.0
    X = np.asarray(it["x3Dw"], np.float32).reshape(-1, 3); out = np.zeros_like(X)
    for j in range(len(X)):
        r = int(it["mp_ref"][j])
        out[j] = [f32(v) for v in SR.smap(Swc[r], SR.smap(g.vScw[r], [F(v) for v in X[j]]))]
    return Siw, Tiw, out


def essential_graph(it, fix_scale):
    """-> the result dict of ORBmatcher.OptimizeEssentialGraph for one item"""
    with np.errstate(all="ignore"):
        g = Graph(it, fix_scale)
        out = dict(n_iters=-1, chi2=F(0.0), lambda_=F(-1.0), n_active=g.n_act, solver_fail=0)
        if g.n_act > 0:
            out["n_iters"], out["chi2"], out["lambda_"] = g.optimize(20, 1e-16)
            out["solver_fail"] = g.fails
        out["Siw"], out["Tiw"], out["x3Dw"] = recover(g, it)
    return out
