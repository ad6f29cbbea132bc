"""Literal Python restatement of the reference's Sim3Solver (src/Sim3Solver.cc) and of the RANSAC loop of LoopClosing::ComputeSim3 (src/LoopClosing.cc:282-342),
one function per reference function.  FP32 steps are numpy float32 scalars (or float32 arrays where a reference loop runs over the correspondences: numpy
neither contracts nor reorders element-wise operations), FP64 steps are Python floats with math.sin / cos / atan2 / sqrt: the libm the host library calls.  The
OpenCV primitives are restated as sindslam_amd/csrc/host/sim3.cpp lists them (OpenCV 4.2.0 as remembered; parity with a real OpenCV is UNPINNED)."""
import math

import numpy as np

F = np.float32
EPS32 = F(np.finfo(np.float32).eps)
DBL_EPSILON = 2.220446049250313e-16


# ---- DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) on a raw rand() value ----
def random_int(raw, lo, hi, rand_max=2147483647):
    d = hi - lo + 1
    return int((float(raw) / (float(rand_max) + 1.0)) * d) + lo


# ---- OpenCV primitives ----
def _hypot(a, b):
    a = abs(a); b = abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(F(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(F(1) + a * a)
    return F(0)


def cv_eigen(Ain):
    """cv::eigen of a symmetric float matrix -> (W descending, V with the eigenvectors as rows): JacobiImpl_<float>"""
    A = [[F(x) for x in row] for row in Ain]
    n = len(A)
    V = [[F(1) if i == j else F(0) for j in range(n)] for i in range(n)]
    W = [F(0)] * n; indR = [0] * n; indC = [0] * n

    def scan_row(r):
        m = r + 1; mv = abs(A[r][m])
        for i in range(r + 2, n):
            val = abs(A[r][i])
            if mv < val: mv, m = val, i
        indR[r] = m

    def scan_col(c):
        m = 0; mv = abs(A[0][c])
        for i in range(1, c):
            val = abs(A[i][c])
            if mv < val: mv, m = val, i
        indC[c] = m

    for k in range(n):
        W[k] = A[k][k]
        if k < n - 1: scan_row(k)
        if k > 0: scan_col(k)
    for _ in range(n * n * 30):
        k = 0; mv = abs(A[0][indR[0]])
        for i in range(1, n - 1):
            val = abs(A[i][indR[i]])
            if mv < val: mv, k = val, i
        l = indR[k]
        for i in range(1, n):
            val = abs(A[indC[i]][i])
            if mv < val: mv, k, l = val, indC[i], i
        p = A[k][l]
        if abs(p) <= EPS32:
            break
        y = F((W[l] - W[k]) * F(0.5))
        t = abs(y) + _hypot(p, y)
        s = _hypot(p, t)
        c = t / s
        s = p / s; t = (p / t) * p
        if y < 0: s, t = -s, -t
        A[k][l] = F(0)
        W[k] = W[k] - t; W[l] = W[l] + t

        def rot(a0, b0):
            return a0 * c - b0 * s, a0 * s + b0 * c
        for i in range(0, k): A[i][k], A[i][l] = rot(A[i][k], A[i][l])
        for i in range(k + 1, l): A[k][i], A[i][l] = rot(A[k][i], A[i][l])
        for i in range(l + 1, n): A[k][i], A[l][i] = rot(A[k][i], A[l][i])
        for i in range(n): V[k][i], V[l][i] = rot(V[k][i], V[l][i])
        for idx in (k, l):
            if idx < n - 1: scan_row(idx)
            if idx > 0: scan_col(idx)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]: m = i
        if k != m:
            W[m], W[k] = W[k], W[m]; V[m], V[k] = V[k], V[m]
    return W, V


def cv_rodrigues(rv):
    """cv::Rodrigues of a float rotation vector -> 3x3 float32, FP64 inside"""
    r = [float(x) for x in rv]
    theta = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta < DBL_EPSILON:
        return np.eye(3, dtype=np.float32)
    c = math.cos(theta) if math.isfinite(theta) else theta / theta; s = math.sin(theta) if math.isfinite(theta) else theta / theta; c1 = 1. - c; itheta = 1. / theta if theta else 0.
    r = [x * itheta for x in r]
    rrt = [r[0] * r[0], r[0] * r[1], r[0] * r[2], r[0] * r[1], r[1] * r[1], r[1] * r[2], r[0] * r[2], r[1] * r[2], r[2] * r[2]]
    rx = [0., -r[2], r[1], r[2], 0., -r[0], -r[1], r[0], 0.]
    eye = [1., 0., 0., 0., 1., 0., 0., 0., 1.]
    return np.array([F((c * eye[i] + c1 * rrt[i]) + s * rx[i]) for i in range(9)], np.float32).reshape(3, 3)


def _small_gemm_row(a, b0, b1, b2, alpha=1.0, c=None, beta=1.0):
    """one element of cv::gemm's small-matrix path: FP32 row product, FP64 alpha / beta"""
    t = a[0] * b0 + a[1] * b1 + a[2] * b2
    return F(float(t) * alpha + float(c) * beta) if c is not None else F(float(t) * alpha)


# ---- Sim3Solver ----
def compute_centroid(P):
    """ComputeCentroid (:215-224): P 3x3 float32, columns are points -> (Pr, C)"""
    third = F(1. / 3)
    C = []
    for r in range(3):
        a0 = P[r][0]; a1 = P[r][1]
        a0 = a0 + P[r][2]; a0 = a0 + a1
        C.append(a0 * third + F(0))
    Pr = [[P[r][c] - C[r] for c in range(3)] for r in range(3)]
    return Pr, C


def compute_sim3(P1, P2, fix_scale):
    """ComputeSim3 (:226-337) -> dict R12 [3,3], t12 [3], s12, T12 [4,4], T21 [4,4], all float32"""
    with np.errstate(all="ignore"):
        P1 = [[F(x) for x in row] for row in P1]; P2 = [[F(x) for x in row] for row in P2]
        Pr1, O1 = compute_centroid(P1); Pr2, O2 = compute_centroid(P2)
        M = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                s = 0.0
                for k in range(3): s += float(Pr2[i][k]) * float(Pr1[j][k])
                M[i][j] = F(s * 1.0)
        N11 = M[0][0] + M[1][1] + M[2][2]; N12 = M[1][2] - M[2][1]; N13 = M[2][0] - M[0][2]; N14 = M[0][1] - M[1][0]
        N22 = M[0][0] - M[1][1] - M[2][2]; N23 = M[0][1] + M[1][0]; N24 = M[2][0] + M[0][2]
        N33 = -M[0][0] + M[1][1] - M[2][2]; N34 = M[1][2] + M[2][1]; N44 = -M[0][0] - M[1][1] + M[2][2]
        N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
        _, evec = cv_eigen(N)
        vec = [evec[0][1], evec[0][2], evec[0][3]]
        nn = 0.0
        for v in vec: nn += float(v) * float(v)
        nrm = math.sqrt(nn) if nn == nn else float("nan")
        ang = math.atan2(nrm, float(evec[0][0]))
        a = F((2 * ang) * (1. / nrm)) if nrm != 0 else F((2 * ang) * float("inf"))
        vec = [v * a + F(0) for v in vec]
        R = cv_rodrigues(vec)
        P3 = [[_small_gemm_row(R[i], Pr2[0][j], Pr2[1][j], Pr2[2][j]) for j in range(3)] for i in range(3)]
        if not fix_scale:
            p = [float(Pr1[i][j]) * float(P3[i][j]) for i in range(3) for j in range(3)]
            nom = 0.0; nom += p[0] + p[1] + p[2] + p[3]; nom += p[4] + p[5] + p[6] + p[7]; nom += p[8]
            den = 0.0
            for i in range(3):
                for j in range(3): den += float(P3[i][j] * P3[i][j])
            s12 = F(nom / den) if den != 0 else F(np.float64(nom) / np.float64(den))
        else:
            s12 = F(1.0)
        t12 = [_small_gemm_row(R[r], O2[0], O2[1], O2[2], alpha=-float(s12), c=O1[r], beta=1.0) for r in range(3)]
        inv = F(np.float64(1.0) / np.float64(s12))
        T12 = np.eye(4, dtype=np.float32); T21 = np.eye(4, dtype=np.float32)
        for r in range(3):
            for c in range(3):
                T12[r, c] = R[r][c] * s12 + F(0); T21[r, c] = R[c][r] * inv + F(0)
            T12[r, 3] = t12[r]
        for r in range(3):
            T21[r, 3] = _small_gemm_row(T21[r], t12[0], t12[1], t12[2], alpha=-1.0)
        return dict(R12=np.array(R, np.float32), t12=np.array(t12, np.float32), s12=F(s12), T12=T12, T21=T21)


def to_camera(T, X):
    """Rcw * X + tcw for [n, 3] float32 points: the small-matrix path of cv::gemm (:95, :98, :396)"""
    T = np.asarray(T, np.float32); X = np.asarray(X, np.float32).reshape(-1, 3)
    out = np.empty_like(X)
    for r in range(3):
        t = T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1] + T[r, 2] * X[:, 2]
        out[:, r] = (t.astype(np.float64) * 1.0 + np.float64(T[r, 3]) * 1.0).astype(np.float32)
    return out


def from_camera_to_image(Xc, K):
    """FromCameraToImage (:405-423) and the tail of Project (:397-401); K = (fx, fy, cx, cy)"""
    fx, fy, cx, cy = [F(v) for v in K]
    with np.errstate(all="ignore"):
        invz = F(1) / Xc[:, 2]
        x = Xc[:, 0] * invz; y = Xc[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], 1)


def project(X, T, K):
    """Project (:382-403)"""
    return from_camera_to_image(to_camera(T, X), K)


def max_error(sigma2):
    """mvnMaxError1/2 (:87-88): size_t, as the float it is compared as"""
    return np.array([F(int(9.210 * float(s))) for s in np.asarray(sigma2, np.float32)], np.float32)


def check_inliers(sv, T12, T21):
    """CheckInliers (:340-364) -> (mvbInliersi, mnInliersi)"""
    with np.errstate(all="ignore"):
        vP2im1 = project(sv["X3Dc2"], T12, sv["K"]); vP1im2 = project(sv["X3Dc1"], T21, sv["K"])
        d1 = sv["P1im1"] - vP2im1; d2 = vP1im2 - sv["P2im2"]
        dot = lambda d: (d[:, 0].astype(np.float64) * d[:, 0].astype(np.float64) + d[:, 1].astype(np.float64) * d[:, 1].astype(np.float64)).astype(np.float32)
        inl = (dot(d1) < sv["maxErr1"]) & (dot(d2) < sv["maxErr2"])
    return inl, int(inl.sum())


def ransac_iterations(n, probability=0.99, min_inliers=20, max_its=300):
    """SetRansacParameters (:114-138) -> mRansacMaxIts; 0 where iterate leaves at :146"""
    if n < min_inliers or n < 1:
        return 0
    epsilon = F(min_inliers) / F(n)
    if min_inliers == n:
        it = 1
    else:
        it = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(epsilon), 3)))
    return max(1, min(it, max_its))


def pack_bits(inl):
    """mvbInliersi as the words sind_match_sim3_ransac returns"""
    n = len(inl); w = np.zeros((n + 63) // 64, np.uint64)
    for i in np.nonzero(inl)[0]:
        w[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return w


class Solver:
    """Sim3Solver.  inp: T1w, T2w, x3Dw1, x3Dw2, sigma2_1, sigma2_2 (per correspondence), indices1 (mvnIndices1), N1 (mN1), K.  `rand` returns raw rand() values."""

    def __init__(self, inp, fix_scale, rand, rand_max=2147483647):
        self.fix, self.rand, self.rand_max = fix_scale, rand, rand_max
        self.mN1 = inp["N1"]; self.idx1 = np.asarray(inp["indices1"], np.int64)
        K = inp["K"]
        X1 = to_camera(inp["T1w"], inp["x3Dw1"]); X2 = to_camera(inp["T2w"], inp["x3Dw2"])
        self.sv = dict(K=K, X3Dc1=X1, X3Dc2=X2, P1im1=from_camera_to_image(X1, K), P2im2=from_camera_to_image(X2, K), maxErr1=max_error(inp["sigma2_1"]), maxErr2=max_error(inp["sigma2_2"]))
        self.N = len(X1)
        self.set_ransac_parameters()
        self.mnBestInliers = 0; self.best = None

    def set_ransac_parameters(self, probability=0.99, min_inliers=20, max_its=300):
        self.minInliers = min_inliers
        self.maxIts = ransac_iterations(self.N, probability, min_inliers, max_its) if self.N >= min_inliers else max_its
        self.mnIterations = 0

    def draw(self):
        avail = list(range(self.N)); out = []
        for _ in range(3):
            randi = random_int(self.rand(), 0, len(avail) - 1, self.rand_max)
            out.append(avail[randi]); avail[randi] = avail[-1]; avail.pop()
        return out

    def hypothesis(self, triple):
        X1, X2 = self.sv["X3Dc1"], self.sv["X3Dc2"]
        P1 = [[X1[triple[c]][r] for c in range(3)] for r in range(3)]; P2 = [[X2[triple[c]][r] for c in range(3)] for r in range(3)]
        return compute_sim3(P1, P2, self.fix)

    def iterate(self, n_iterations):
        """-> (Scm or None, bNoMore, vbInliers [mN1], nInliers)"""
        vb = np.zeros(self.mN1, bool)
        if self.N < self.minInliers:
            return None, True, vb, 0
        cur = 0
        while self.mnIterations < self.maxIts and cur < n_iterations:
            cur += 1; self.mnIterations += 1
            h = self.hypothesis(self.draw())
            inl, cnt = check_inliers(self.sv, h["T12"], h["T21"])
            if cnt >= self.mnBestInliers:
                self.mnBestInliers = cnt; self.best = dict(h, inliers=inl)
                if cnt > self.minInliers:
                    vb[self.idx1[inl]] = True
                    return h["T12"], False, vb, cnt
        return None, self.mnIterations >= self.maxIts, vb, 0


def compute_sim3_loop(solvers, accept):
    """LoopClosing::ComputeSim3's while loop (:282-342).  solvers[i] None = vbDiscarded[i] on entry.  accept(i, Scm, vbInliers) stands for SearchBySim3 + OptimizeSim3
    and returns whether nInliers >= 20.  -> (matched candidate or -1, Scm or None, vbInliers or None, vbDiscarded, log of (i, Scm bits, vbInliers, accepted))"""
    discarded = [s is None for s in solvers]
    n_cand = sum(not d for d in discarded)
    log = []
    while n_cand > 0:
        for i, s in enumerate(solvers):
            if discarded[i]:
                continue
            Scm, no_more, vb, n_in = s.iterate(5)
            if no_more:
                discarded[i] = True; n_cand -= 1
            if Scm is not None:
                ok = bool(accept(i, Scm, vb))
                log.append((i, Scm.copy(), vb.copy(), ok))
                if ok:
                    return i, Scm, vb, discarded, log
    return -1, None, None, discarded, log
