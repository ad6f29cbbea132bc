"""Key-frame cloud generation of the mapping consumer — Python mirror of generatePointCloud(imgRGB, imgDepth, imgDepthLast, imgDynaMask,
imgDynaMaskLast, imgLabel, poseRelative, Twc) (reference octomap_pub/src/pubPointCloud.cc:471-668) over the C ABI, and of the statistical outlier
filter that follows it there (:291-296; sind_cloud_filter_outliers, contract in include/sind_hip.h, parity with a real PCL build unpinned)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import SindError, check, lib, ptr

POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])
STATS_DTYPE = np.dtype([("mean", "f8"), ("stddev", "f8"), ("threshold", "f8"), ("valid", "i4"), ("degenerate", "i4"), ("n_ring", "i4"), ("n_brute", "i4")])
MAX_MEAN_K = 128                                                       # sind_cloud_filter_max_mean_k()

_host = None


def _host_lib():
    """libsind_host.so: the host twin sindh_cloud_filter_outliers (the arithmetic of csrc/host/cloud_filter.hpp over its own search)"""
    global _host
    if _host is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsind_host.so")
        if not os.path.exists(path):
            raise SindError(f"{path} not built")
        _host = C.CDLL(path)
    return _host


def _pack(points_list):
    pl = [np.ascontiguousarray(p, POINT_DTYPE) for p in points_list]
    n = np.array([len(p) for p in pl], np.int32); stride = max(1, int(n.max()) if len(pl) else 1)
    pts = np.zeros((len(pl), stride), POINT_DTYPE)
    for b, p in enumerate(pl):
        pts[b, :len(p)] = p
    return pts, n, stride


def _unpack(B, n, out, n_out, dist, stats):
    return [dict(points=out[b, :n_out[b]].copy(), distances=dist[b, :n[b]].copy(), mean=float(stats[b]["mean"]), stddev=float(stats[b]["stddev"]),
                 threshold=float(stats[b]["threshold"]), valid=int(stats[b]["valid"]), degenerate=int(stats[b]["degenerate"]), n_ring=int(stats[b]["n_ring"]),
                 n_brute=int(stats[b]["n_brute"]), stats=stats[b].copy()) for b in range(B)]


def filterOutliersHost(points_list, mean_k=100, stddev_mul=1.0):
    """The host twin of CloudGenerator.filterOutliers: no device, no handle.  Same result, bit for bit (n_ring = n_brute = 0)."""
    pts, n, stride = _pack(points_list); B = len(n)
    out = np.zeros((B, stride), POINT_DTYPE); n_out = np.zeros(max(B, 1), np.int32); dist = np.zeros((B, stride), np.float32); stats = np.zeros(max(B, 1), STATS_DTYPE)
    rc = _host_lib().sindh_cloud_filter_outliers(B, ptr(pts), stride, ptr(n), int(mean_k), C.c_double(stddev_mul), ptr(out), stride, ptr(n_out), ptr(dist), ptr(stats))
    if rc < 0:
        raise SindError(f"sindh_cloud_filter_outliers failed ({rc})")
    return _unpack(B, n, out, n_out, dist, stats)


class CloudGenerator:
    def __init__(self, fx, fy, cx, cy, depth_scale, width=640, height=480, max_batch=1, device=0):
        h = C.c_void_p()
        check(lib().sind_cloud_create(C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), C.c_double(depth_scale), width, height,
                                      max_batch, device, C.byref(h)), "sind_cloud_create")
        self._h = h; self.width, self.height, self.max_batch = width, height, max_batch
        self.cap = lib().sind_cloud_max_points(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().sind_cloud_destroy(self._h); self._h = None

    __del__ = close

    def generatePointCloud(self, imgRGB, imgDepth, imgDepthLast, imgDynaMask, imgDynaMaskLast, imgLabel, poseRelative, Twc, filter=None):
        """All images [B, H, W(, 3)]; poses [B, 4, 4] float64 -> list of dict(points, occlusion, label_count, kept).
        filter=True or filter=(mean_k, stddev_mul) also runs the statistical outlier filter (pubPointCloud.cc:291-296; True = the reference's 100, 1.0) on the clouds
        the call left on the device: each dict then holds temp1 = dict(points, distances, mean, stddev, threshold, ...) beside tempCloudOneFrame in points."""
        B = len(imgDepth)
        u8 = lambda a: np.ascontiguousarray(a, np.uint8); u16 = lambda a: np.ascontiguousarray(a, np.uint16); f64 = lambda a: np.ascontiguousarray(a, np.float64)
        bgr, d, dl, m, ml, lb, pr, tw = u8(imgRGB), u16(imgDepth), u16(imgDepthLast), u8(imgDynaMask), u8(imgDynaMaskLast), u8(imgLabel), f64(poseRelative), f64(Twc)
        assert bgr.shape == (B, self.height, self.width, 3) and d.shape == dl.shape == m.shape == ml.shape == lb.shape == (B, self.height, self.width)
        assert pr.shape == tw.shape == (B, 4, 4)
        pts = np.zeros((B, self.cap), POINT_DTYPE); n = np.zeros(B, np.int32)
        occ = np.zeros((B, 12), np.int32); cnt = np.zeros((B, 12), np.int32); kept = np.zeros((B, 12), np.int32)
        check(lib().sind_cloud_generate(self._h, B, ptr(bgr), ptr(d), ptr(dl), ptr(m), ptr(ml), ptr(lb), ptr(pr), ptr(tw), 0, ptr(pts), self.cap, ptr(n),
                                        ptr(occ), ptr(cnt), ptr(kept)), "sind_cloud_generate")
        res = [dict(points=pts[b, :n[b]].copy(), occlusion=occ[b], label_count=cnt[b], kept=kept[b]) for b in range(B)]
        if filter:
            mean_k, mul = (100, 1.0) if filter is True else filter
            for r, t in zip(res, self._filter(B, None, self.cap, n, mean_k, mul)):
                r["temp1"] = t
        return res

    def _filter(self, B, pts, stride, n, mean_k, stddev_mul):
        out = np.zeros((B, stride), POINT_DTYPE); n_out = np.zeros(B, np.int32); dist = np.zeros((B, stride), np.float32); stats = np.zeros(B, STATS_DTYPE)
        check(lib().sind_cloud_filter_outliers(self._h, B, ptr(pts), stride, ptr(n), 0, int(mean_k), C.c_double(stddev_mul), ptr(out), stride, ptr(n_out), ptr(dist),
                                               ptr(stats)), "sind_cloud_filter_outliers")
        return _unpack(B, n, out, n_out, dist, stats)

    def filterOutliers(self, points_list, mean_k=100, stddev_mul=1.0, host=False):
        """pcl::StatisticalOutlierRemoval (setMeanK, setStddevMulThresh, filter) on up to max_batch clouds of POINT_DTYPE at once -> list of dict(points = the kept
        points in input order, distances [n], mean, stddev, threshold, valid, degenerate, n_ring, n_brute).  host=True runs the host twin instead."""
        if host:
            return filterOutliersHost(points_list, mean_k, stddev_mul)
        pts, n, stride = _pack(points_list)
        return self._filter(len(n), pts, stride, n, mean_k, stddev_mul)
