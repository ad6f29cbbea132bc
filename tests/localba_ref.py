"""Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:506-778) restated in Python with NumPy FP64 scalars, operation for operation in the order that the head
of sindslam_amd/csrc/host/ba_schur.hpp states (vertex order, edge order, the ordered sums, the Schur loop nest, the dense LDL^T, back-substitution); the pose algebra,
the edge errors and the Huber kernel are poseopt_ref's.  Plain sequential loops over plain lists, for small scenes only.  Bit equality with the host library is BY
CONSTRUCTION of the two texts; tests/test_localba_cpu.py asserts it and checks the result against things that are neither."""
from __future__ import annotations

import numpy as np

import poseopt_ref as PR
from poseopt_ref import DBL_MAX, F, ONE, ZERO, f32

DP = (0, 6, 11, 15, 18, 20)                                            # the diagonal of an upper 6 x 6 stored by rows
DL = (0, 3, 5)


def cof(m, i, j):
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1]


def inv3(m):
    c0, c1, c2 = cof(m, 0, 0), cof(m, 1, 0), cof(m, 2, 0)
    det = c0 * m[0][0] + c1 * m[1][0] + c2 * m[2][0]
    invdet = ONE / det
    return [[c0 * invdet, c1 * invdet, c2 * invdet]] + [[cof(m, j, i) * invdet for j in range(3)] for i in (1, 2)]


def edge(P, K, X, ob, robust, full, pose_free):
    """-> dict(rho0, chi2) and, if full, Hl [6], bl [3] and, if pose_free, Hp [21], bp [6], Hpl [6][3]; A, B, e for the tests"""
    fx, fy, cx, cy, bf = K
    stereo = not (ob[2] < f32(0.0))
    s = F(ob[3])
    chi2, e, Xc = PR.edge_error(P, K, X, F(ob[0]), F(ob[1]), F(ob[2]), stereo, s)
    rho0, rho1 = chi2, ONE
    if robust:
        rho0, rho1 = PR.huber(chi2, PR.DELTA[stereo])
    c = dict(rho0=rho0, chi2=chi2)
    if not full:
        return c
    R = PR.quat_to_matrix(P[0])
    x, y, z = Xc; z_2 = z * z
    if not stereo:
        tmp = [[fx, ZERO, -x / z * fx], [ZERO, fy, -y / z * fy]]
        m = F(-1.0) / z
        A = [[(m * tmp[r][0]) * R[0][q] + (m * tmp[r][1]) * R[1][q] + (m * tmp[r][2]) * R[2][q] for q in range(3)] for r in range(2)] + [[ZERO] * 3]
    else:
        A = [[None] * 3 for _ in range(3)]
        for q in range(3):
            A[0][q] = -fx * R[0][q] / z + fx * x * R[2][q] / z_2
            A[1][q] = -fy * R[1][q] / z + fy * y * R[2][q] / z_2
            A[2][q] = A[0][q] - bf * R[2][q] / z_2
    B = [[x * y / z_2 * fx, -(ONE + (x * x / z_2)) * fx, y / z * fx, F(-1.0) / z * fx, ZERO, x / z_2 * fx],
         [(ONE + y * y / z_2) * fy, -x * y / z_2 * fy, -x / z * fy, ZERO, F(-1.0) / z * fy, y / z_2 * fy], [ZERO] * 6]
    if stereo:
        B[2] = [B[0][0] - bf * y / z_2, B[0][1] + bf * x / z_2, B[0][2], B[0][3], ZERO, B[0][5] - bf / z_2]
    c.update(A=A, B=B, e=e)
    W = rho1 * s if robust else s
    wr = [-(s * e[d]) for d in range(3)]
    if robust:
        wr = [v * rho1 for v in wr]

    def quad(J1, i, J2, j):
        h = (J1[0][i] * W) * J2[0][j] + (J1[1][i] * W) * J2[1][j]
        return h + (J1[2][i] * W) * J2[2][j] if stereo else h

    def lin(J, j):
        t = J[0][j] * wr[0] + J[1][j] * wr[1]
        return t + J[2][j] * wr[2] if stereo else t

    c["Hl"] = [quad(A, i, A, j) for i in range(3) for j in range(i, 3)]
    c["bl"] = [lin(A, j) for j in range(3)]
    if pose_free:
        c["Hp"] = [quad(B, i, B, j) for i in range(6) for j in range(i, 6)]
        c["bp"] = [lin(B, j) for j in range(6)]
        c["Hpl"] = [[quad(B, r, A, q) for q in range(3)] for r in range(6)]
    return c


class Graph:
    def __init__(self, it, K):
        self.K = [F(f32(k)) for k in K]
        self.n_kf, self.n_mp = len(it["kf_id"]), len(it["mp_id"])
        self.kind = [int(k) for k in it["kf_kind"]]
        free = sorted([k for k in range(self.n_kf) if self.kind[k] == 0], key=lambda k: int(it["kf_id"][k]))
        self.pose_kf = free; self.P = len(free)
        self.kf_pose = [-1] * self.n_kf
        for s, k in enumerate(free):
            self.kf_pose[k] = s
        self.pt_order = sorted(range(self.n_mp), key=lambda j: int(it["mp_id"][j]))
        self.obs_start = [int(v) for v in it["obs_start"]] if self.n_mp else [0]
        self.n_obs = self.obs_start[-1]
        self.e_kf = [int(v) for v in it["obs_kf"]]
        self.e_pt = [j for j in range(self.n_mp) for _ in range(self.obs_start[j], self.obs_start[j + 1])]
        self.ob = [(f32(it["obs_xy"][e][0]), f32(it["obs_xy"][e][1]), f32(it["u_right"][e]), f32(it["inv_sigma2"][e])) for e in range(self.n_obs)]
        self.pose_edges = [[e for e in range(self.n_obs) if self.kf_pose[self.e_kf[e]] == s] for s in range(self.P)]
        self.pt_sorted = [sorted([e for e in range(self.obs_start[j], self.obs_start[j + 1]) if self.kf_pose[self.e_kf[e]] >= 0], key=lambda e: self.kf_pose[self.e_kf[e]]) for j in range(self.n_mp)]
        self.est = [PR.from_tcw(it["Tcw"][k]) for k in range(self.n_kf)]
        self.X = [[F(f32(v)) for v in it["x3Dw"][j]] for j in range(self.n_mp)]
        self.level = [0] * self.n_obs
        self.C = [dict(chi2=ZERO) for _ in range(self.n_obs)]
        self.x = []

    def rank(self, e):
        return self.kf_pose[self.e_kf[e]]

    def evaluate(self, robust, full):
        for e in range(self.n_obs):
            if not self.level[e]:
                k = self.e_kf[e]
                self.C[e].update(edge(self.est[k], self.K, self.X[self.e_pt[e]], self.ob[e], robust, full, self.kf_pose[k] >= 0))      # a trial rewrites rho[0] and chi2 alone

    def sums(self):
        self.Hpp = [[ZERO] * 27 for _ in range(self.P)]
        for s in range(self.P):
            for e in self.pose_edges[s]:
                if not self.level[e]:
                    c = self.C[e]
                    self.Hpp[s] = [a + b for a, b in zip(self.Hpp[s], c["Hp"] + c["bp"])]
        self.Hll = [[ZERO] * 9 for _ in range(self.n_mp)]
        for j in range(self.n_mp):
            for e in range(self.obs_start[j], self.obs_start[j + 1]):
                if not self.level[e]:
                    c = self.C[e]
                    self.Hll[j] = [a + b for a, b in zip(self.Hll[j], c["Hl"] + c["bl"])]

    def chi(self):
        s = ZERO
        for e in range(self.n_obs):
            if not self.level[e]:
                s = s + self.C[e]["rho0"]
        return s

    def activate(self):
        self.pose_idx = []; k = 0
        for s in range(self.P):
            act = any(not self.level[e] for e in self.pose_edges[s])
            self.pose_idx.append(k if act else -1); k += 1 if act else 0
        self.n_act = k
        self.pt_act = [any(not self.level[e] for e in range(self.obs_start[j], self.obs_start[j + 1])) for j in range(self.n_mp)]
        return k + sum(self.pt_act)

    def max_diagonal(self):
        m = ZERO
        for s in range(self.P):
            if self.pose_idx[s] >= 0:
                for j in range(6):
                    a = np.abs(self.Hpp[s][DP[j]]); m = m if a < m else a
        for q in self.pt_order:
            if self.pt_act[q]:
                for j in range(3):
                    a = np.abs(self.Hll[q][DL[j]]); m = m if a < m else a
        return m

    def solve(self, lam):
        """-> False on a zero pivot (x untouched)"""
        n = 6 * self.n_act
        Dinv, db = [None] * self.n_mp, [None] * self.n_mp
        for j in range(self.n_mp):
            if self.pt_act[j]:
                h = self.Hll[j]
                Dinv[j] = inv3([[h[0] + lam, h[1], h[2]], [h[1], h[3] + lam, h[4]], [h[2], h[4], h[5] + lam]])
                db[j] = [Dinv[j][r][0] * h[6] + Dinv[j][r][1] * h[7] + Dinv[j][r][2] * h[8] for r in range(3)]
        BD = {}
        for e in range(self.n_obs):
            if not self.level[e] and self.rank(e) >= 0:
                Bi, Di = self.C[e]["Hpl"], Dinv[self.e_pt[e]]
                BD[e] = [[Bi[r][0] * Di[0][q] + Bi[r][1] * Di[1][q] + Bi[r][2] * Di[2][q] for q in range(3)] for r in range(6)]
        Hs = [[ZERO] * n for _ in range(n)]
        co = [ZERO] * n
        for s in range(self.P):                                        # Hschur = Hpp with lambda on the diagonal blocks
            i = self.pose_idx[s]
            if i >= 0:
                for r in range(6):
                    for q in range(r, 6):
                        v = self.Hpp[s][r * 6 - r * (r - 1) // 2 + (q - r)]
                        Hs[6 * i + r][6 * i + q] = v + lam if r == q else v
        for j in self.pt_order:                                        # the loop nest of block_solver.hpp:381-439: ascending landmark, its pose blocks in ascending row
            if not self.pt_act[j]:
                continue
            col = [e for e in self.pt_sorted[j] if not self.level[e]]
            for a, e1 in enumerate(col):
                i1 = self.pose_idx[self.rank(e1)]; Bi = self.C[e1]["Hpl"]
                for r in range(6):
                    co[6 * i1 + r] = co[6 * i1 + r] + (Bi[r][0] * db[j][0] + Bi[r][1] * db[j][1] + Bi[r][2] * db[j][2])
                for e2 in col[a:]:
                    i2 = self.pose_idx[self.rank(e2)]; Bj = self.C[e2]["Hpl"]
                    for r in range(6):
                        for q in range(6):
                            if i1 == i2 and r > q:
                                continue
                            Hs[6 * i1 + r][6 * i2 + q] = Hs[6 * i1 + r][6 * i2 + q] - (BD[e1][r][0] * Bj[q][0] + BD[e1][r][1] * Bj[q][1] + BD[e1][r][2] * Bj[q][2])
        y = [ZERO] * n
        for s in range(self.P):
            i = self.pose_idx[s]
            if i >= 0:
                for r in range(6):
                    y[6 * i + r] = self.Hpp[s][21 + r] - co[6 * i + r]
        L = [[ZERO] * n for _ in range(n)]; D = [ZERO] * n
        with np.errstate(all="ignore"):
            for j in range(n):
                for i in range(j, n):
                    v = Hs[j][i]
                    for k in range(j):
                        v = v - (L[i][k] * D[k]) * L[j][k]
                    if i == j:
                        D[j] = v
                    else:
                        L[i][j] = v / D[j]
        if any(d == 0.0 for d in D):
            return False
        for j in range(n):
            for i in range(j + 1, n):
                y[i] = y[i] - L[i][j] * y[j]
        y = [y[i] / D[i] for i in range(n)]
        for j in range(n - 1, 0, -1):
            for i in range(j):
                y[i] = y[i] - L[j][i] * y[j]
        for s in range(self.P):
            i = self.pose_idx[s]
            if i >= 0:
                self.x[6 * s:6 * s + 6] = y[6 * i:6 * i + 6]
        for j in range(self.n_mp):
            if not self.pt_act[j]:
                continue
            cl = list(self.Hll[j][6:9])
            for e in self.pt_sorted[j]:
                if self.level[e]:
                    continue
                Bi = self.C[e]["Hpl"]; xp = self.x[6 * self.rank(e):6 * self.rank(e) + 6]
                for q in range(3):
                    t = Bi[0][q] * -xp[0]
                    for r in range(1, 6):
                        t = t + Bi[r][q] * -xp[r]
                    cl[q] = cl[q] + t
            for r in range(3):
                self.x[6 * self.P + 3 * j + r] = ZERO + (Dinv[j][r][0] * cl[0] + Dinv[j][r][1] * cl[1] + Dinv[j][r][2] * cl[2])
        return True

    def update(self):
        for s in range(self.P):
            if self.pose_idx[s] >= 0:
                self.est[self.pose_kf[s]] = PR.oplus(self.x[6 * s:6 * s + 6], self.est[self.pose_kf[s]])
        for j in range(self.n_mp):
            if self.pt_act[j]:
                self.X[j] = [self.X[j][k] + self.x[6 * self.P + 3 * j + k] for k in range(3)]

    def scale(self, lam):
        sc = ZERO
        for s in range(self.P):
            if self.pose_idx[s] >= 0:
                for j in range(6):
                    xj = self.x[6 * s + j]; sc = sc + xj * (lam * xj + self.Hpp[s][21 + j])
        for q in self.pt_order:
            if self.pt_act[q]:
                for j in range(3):
                    xj = self.x[6 * self.P + 3 * q + j]; sc = sc + xj * (lam * xj + self.Hll[q][6 + j])
        return sc

    def bad(self, e):
        stereo = not (self.ob[e][2] < f32(0.0))
        z = PR.se3_map(self.est[self.e_kf[e]], self.X[self.e_pt[e]])[2]
        return bool(self.C[e]["chi2"] > (F(7.815) if stereo else F(5.991)) or not (z > 0.0))

    def optimize(self, robust, iterations):
        self.x = [ZERO] * (6 * self.P + 3 * self.n_mp)
        lam, ni, current, cj, n_bad, ok = F(-1.0), F(2.0), ZERO, 0, 0, True
        i = 0
        while i < iterations and ok:
            self.evaluate(robust, True); self.sums()
            current = self.chi(); temp = current; ini = current
            if i == 0:
                lam = F(1e-5) * self.max_diagonal(); ni = F(2.0); n_bad = 0
            rho, qmax = ZERO, 0
            while True:
                backup = (list(self.est), [list(v) for v in self.X])
                ok2 = self.solve(lam)
                self.update()
                self.evaluate(robust, False)
                temp = self.chi()
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
                    lam = lam * ni; ni = ni * F(2.0); self.est, self.X = backup
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


def local_ba(it, K):
    """-> the result dict of ORBmatcher.LocalBundleAdjustment for one item"""
    with np.errstate(all="ignore"):
        g = Graph(it, K)
        out = dict(n_stages=0, n_level1=0, stage_iters=np.zeros(2, np.int32), stage_chi2=np.zeros(2), stage_lambda=np.zeros(2))
        for s in range(2):
            if s == 1:
                if not it.get("do_more", True):
                    break
                for e in range(g.n_obs):
                    if g.bad(e):
                        g.level[e] = 1
                out["n_level1"] = sum(g.level)
            if g.activate() == 0:
                continue
            out["stage_iters"][s], out["stage_chi2"][s], out["stage_lambda"][s] = g.optimize(s == 0, 5 if s == 0 else 10)
            out["n_stages"] += 1
        out["erase"] = np.array([g.bad(e) for e in range(g.n_obs)], np.uint8)
        out["Tcw"] = np.array([np.asarray(it["Tcw"][k], np.float32).reshape(4, 4) if g.kind[k] == 2 else PR.to_tcw(g.est[k]) for k in range(g.n_kf)], np.float32).reshape(g.n_kf, 4, 4)
        out["x3Dw"] = np.array([[f32(v) for v in g.X[j]] for j in range(g.n_mp)], np.float32).reshape(g.n_mp, 3)
    return out
