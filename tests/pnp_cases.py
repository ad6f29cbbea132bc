"""Shared by test_pnp_cpu.py and test_pnp_gpu.py: the host library's PnP entry points (sindh_pnp_*, csrc/host/pnp.cpp), bit patterns, and the special samples."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = lambda a: C.c_void_p(a.ctypes.data)
_host = None
# per number of correspondences, ten times the largest deviation from the ground-truth pose (rotation, translation) that
# test_pnp_cpu.py::test_pose_recovers_the_ground_truth_without_noise measured over its 50 seeds (its docstring has the figures)
BOUNDS = {6: (1.938e-6, 1.162e-5), 20: (7.986e-7, 4.274e-6), 100: (3.367e-7, 2.189e-6)}
BOUND_R, BOUND_T = BOUNDS[6]                                            # the loosest: for a pose from a set of another size (the chain test)


def host():
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(ROOT, "sindslam_amd", "libsind_host.so"))
    return _host


def calib(K):
    """fu fv uc vc as the library reads them: the FP64 of the FP32 the handle holds"""
    return [float(np.float32(k)) for k in K]


def bits64(a):
    """bit patterns of FP64, every NaN as one pattern: which NaN an operation returns is the processor's choice and decides nothing (no comparison with it holds)"""
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.uint64(0x7ff8000000000000), a.view(np.uint64))


def host_pose(x3Dw, p2d, K):
    """sindh_pnp_pose -> R [3, 3], t [3], reprojection error"""
    x = np.ascontiguousarray(x3Dw, np.float32); u = np.ascontiguousarray(p2d, np.float32)
    R = np.zeros((3, 3)); t = np.zeros(3); e = np.zeros(1)
    host().sindh_pnp_pose(len(x), _P(x), _P(u), *[C.c_double(k) for k in calib(K)], _P(R), _P(t), _P(e))
    return R, t, float(e[0])


def host_check(inp, K, R, t):
    """sindh_pnp_check -> (count, bits u64 [ceil(n / 64)])"""
    x = np.ascontiguousarray(inp["x3Dw"], np.float32); u = np.ascontiguousarray(inp["p2d"], np.float32); s = np.ascontiguousarray(inp["sigma2"], np.float32)
    R = np.ascontiguousarray(R, np.float64); t = np.ascontiguousarray(t, np.float64); w = np.zeros(max((len(s) + 63) // 64, 1), np.uint64)
    cnt = host().sindh_pnp_check(len(s), _P(x), _P(u), _P(s), C.c_float(inp["th2"]), *[C.c_double(k) for k in calib(K)], _P(R), _P(t), _P(w))
    return int(cnt), w[:(len(s) + 63) // 64]


def host_refine_plan(counts, min_inliers, best_count, has_best):
    c = np.ascontiguousarray(counts, np.int32); of_hyp = np.zeros(max(len(c), 1), np.int32); hyps = np.zeros(len(c) + 1, np.int32)
    n = host().sindh_pnp_refine_plan(_P(c), len(c), int(min_inliers), int(best_count), int(has_best), _P(of_hyp), _P(hyps))
    return list(of_hyp[:len(c)]), list(hyps[:n])


def host_evaluate(K):
    """what sind_match_pnp_ransac computes, by the host entry points alone (the same source as the device's): an `evaluate` for sindslam_amd.pnp.PnPsolver"""
    import pnp_ref as P

    def one(inp, samples, min_inliers, best_count, best_bits):
        n = len(inp["sigma2"]); w = (n + 63) // 64
        hs = []
        for s in samples:
            R, t, _ = host_pose(inp["x3Dw"][list(s)], inp["p2d"][list(s)], K)
            hs.append((R, t) + host_check(inp, K, R, t))
        of_hyp, hyps = host_refine_plan([h[2] for h in hs], min_inliers, best_count, best_bits is not None)
        rs = []
        for h in hyps:
            idx = np.flatnonzero(P.unpack_bits(best_bits if h < 0 else hs[h][3], n))
            R, t, _ = host_pose(inp["x3Dw"][idx], inp["p2d"][idx], K)
            rs.append((R, t) + host_check(inp, K, R, t))
        arr = lambda rows, k, shape, dt: np.array([r[k] for r in rows], dt).reshape((len(rows),) + shape)
        return dict(count=arr(hs, 2, (), np.int32), bits=arr(hs, 3, (w,), np.uint64), R=arr(hs, 0, (3, 3), np.float64), t=arr(hs, 1, (3,), np.float64), refine=np.array(of_hyp, np.int32),
                    refine_hyp=np.array(hyps, np.int32), refine_count=arr(rs, 2, (), np.int32), refine_bits=arr(rs, 3, (w,), np.uint64), refine_R=arr(rs, 0, (3, 3), np.float64),
                    refine_t=arr(rs, 1, (3,), np.float64))
    return lambda requests: [one(*r) for r in requests]


def zero_depth_point(R, t):
    """float32 (X, Y, Z) for which CheckInliers' R[2][0] * X + R[2][1] * Y + R[2][2] * Z + t[2], in FP64 and in that order, is exactly 0: Z cancels t[2] to FP32 precision,
    X what is left of it, Y the rest; then a search among Y's neighbours"""
    f = lambda v: float(np.float32(v))
    r6, r7, r8 = (float(v) for v in R[2]); t2 = float(t[2])
    depth = lambda X, Y, Z: ((r6 * X + r7 * Y) + r8 * Z) + t2
    Z = f(-t2 / r8)
    X = f(-depth(0.0, 0.0, Z) / r6)
    for _ in range(64):
        Y = f(-depth(X, 0.0, Z) / r7)
        lo = hi = np.float32(Y)
        for _ in range(64):
            for c in (lo, hi):
                if depth(X, float(c), Z) == 0:
                    return np.array([X, float(c), Z], np.float32)
            lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
        X = float(np.nextafter(np.float32(X), np.float32(np.inf)))
    raise AssertionError("no float point of depth exactly 0 for this pose")


def special_samples(K):
    """name -> (x3Dw [4, 3], p2d [4, 2]): the degenerate 4-point problems"""
    import pnp_scene as S
    c = S.candidate(11, 12, outliers=0, noise=0)
    X, U = c["x3Dw"].copy(), c["p2d"].copy()
    proj = lambda Xw: np.stack([K[2] + K[0] * (Xw @ c["R"].T + c["t"])[:, 0] / (Xw @ c["R"].T + c["t"])[:, 2], K[3] + K[1] * (Xw @ c["R"].T + c["t"])[:, 1] / (Xw @ c["R"].T + c["t"])[:, 2]], 1)
    out = {}
    P = X[:4].astype(np.float64); P[3] = P[0] + 0.3 * (P[1] - P[0]) + 0.6 * (P[2] - P[0])             # four coplanar points
    out["coplanar"] = (P.astype(np.float32), proj(P.astype(np.float32).astype(np.float64)).astype(np.float32))
    P = X[:4].astype(np.float64); P[2] = P[0] + 0.5 * (P[1] - P[0])                                     # three collinear points and one more
    out["collinear"] = (P.astype(np.float32), proj(P.astype(np.float32).astype(np.float64)).astype(np.float32))
    P, Q = X[:4].copy(), U[:4].copy(); P[2] = P[0]; Q[2] = Q[0]                                          # two identical points
    out["repeated"] = (P, Q)
    P, Q = X[4:8].copy(), U[4:8].copy()
    P[1] = (-c["R"].T @ c["t"]).astype(np.float32); Q[1] = (K[2], K[3])                                  # a point at the camera centre
    out["centre"] = (P, Q)
    P, Q = X[4:8].copy(), U[4:8].copy(); P[:] = P[0]; Q[:] = Q[0]                                        # one point four times: every matrix is zero
    out["all_equal"] = (P, Q)
    return out
