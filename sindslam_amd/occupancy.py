"""Occupancy map of the mapping consumer — Python mirror of the octree part of the reference's key-frame callback (octomap_pub/src/pubPointCloud.cc:299-365:
insertRay per point, integrateNodeColor per point, the walk over the occupied leaves) over the C ABI (sind_occmap_*, contract in include/sind_hip.h).  The contract is
restated from octomap 1.9 as recalled; parity with a real octomap build is unpinned.  The map is flat (depth 16 only, no pruning)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import SindError, check, lib, ptr
from .cloud import POINT_DTYPE, _host_lib, _pack

OCC_STATS_DTYPE = np.dtype([("n_rays", "i4"), ("n_skipped", "i4"), ("n_coloured", "i4"), ("n_miss_updates", "i4"), ("n_new_voxels", "i4")])
KEY_OFFSET = 32768


class OccupancyMap:
    """host=True builds the host twin (libsind_host.so: the literal sequential loops, no device) behind the same methods."""

    def __init__(self, resolution=0.02, prob_hit=0.7, prob_miss=0.4, clamp_min=0.1192, clamp_max=0.971, occ_thres=0.7, max_voxels=1 << 22, max_points=76800,
                 device=0, host=False):
        self.host = bool(host); self.resolution = float(resolution); self.max_voxels, self.max_points = int(max_voxels), int(max_points)
        self._L = _host_lib() if host else lib(); self._pre = "sindh_occmap_" if host else "sind_occmap_"
        h = C.c_void_p()
        args = [C.c_double(v) for v in (resolution, prob_hit, prob_miss, clamp_min, clamp_max, occ_thres)] + [self.max_voxels, self.max_points]
        self._check(self._f("create")(*args, *(() if host else (device,)), C.byref(h)), "create")
        self._h = h

    def _f(self, name):
        return getattr(self._L, self._pre + name)

    def _check(self, rc, what):
        if rc < 0 and self.host:
            raise SindError(f"{self._pre}{what} failed ({rc})")
        return check(rc, self._pre + what)

    def close(self):
        if getattr(self, "_h", None):
            self._f("destroy")(self._h); self._h = None

    __del__ = close

    def clear(self):
        self._check(self._f("clear")(self._h), "clear")

    @property
    def size(self):
        """the number of known voxels (not octomap's size(), which counts inner nodes)"""
        return self._check(self._f("size")(self._h), "size")

    def insert(self, points_list, origins, host=False):
        """insertRay(origin, p) for every point with p.z >= 0 of each cloud (POINT_DTYPE), then integrateNodeColor for every point; B clouds equal B calls in order.
        origins [B, 3] -> stats [B] of OCC_STATS_DTYPE.  host=True is only legal on a host=True map (there is one state, it lives on one side)."""
        if host and not self.host:
            raise SindError("OccupancyMap.insert(host=True) needs a map created with host=True")
        pts, n, stride = _pack(points_list); B = len(n)
        org = np.ascontiguousarray(origins, np.float32).reshape(B, 3); stats = np.zeros(max(B, 1), OCC_STATS_DTYPE)
        if self.host:
            rc = self._f("insert")(self._h, B, ptr(pts), stride, ptr(n), ptr(org), ptr(stats))
        else:
            rc = self._f("insert")(self._h, B, ptr(pts), stride, ptr(n), ptr(org), 0, ptr(stats))
        self._check(rc, "insert")
        return stats[:B]

    def insertGenerated(self, generator, Twc):
        """the clouds that generator's last generatePointCloud left on the device (the UNFILTERED tempCloudOneFrame, as the reference inserts), origin = Twc[:, :3, 3]
        cast to float (:303)"""
        if self.host:
            raise SindError("OccupancyMap.insertGenerated reads device memory: not on a host=True map")
        Twc = np.asarray(Twc, np.float64).reshape(-1, 4, 4); B = len(Twc)
        org = np.ascontiguousarray(Twc[:, :3, 3], np.float32); stats = np.zeros(B, OCC_STATS_DTYPE)
        self._check(self._f("insert_generated")(self._h, generator._h, B, ptr(org), ptr(stats)), "insert_generated")
        return stats

    def occupied(self):
        """every known voxel with logodds >= occ_thres as POINT_DTYPE (voxel centre, colour), in octomap's leaf_iterator order"""
        n = np.zeros(1, np.int32)
        self._check(self._f("occupied")(self._h, None, 0, ptr(n)), "occupied")
        out = np.zeros(max(int(n[0]), 1), POINT_DTYPE)
        self._check(self._f("occupied")(self._h, ptr(out), len(out), ptr(n)), "occupied")
        return out[:int(n[0])]

    def read(self, keys):
        """keys [n, 3] uint16 -> known [n] u1, logodds [n] f4, rgb [n, 3] u1 (zeros where unknown)"""
        k = np.ascontiguousarray(keys, np.uint16).reshape(-1, 3); n = len(k)
        known = np.zeros(n, np.uint8); lo = np.zeros(n, np.uint32); rgb = np.zeros((n, 3), np.uint8)
        self._check(self._f("read")(self._h, ptr(k), n, ptr(known), ptr(lo), ptr(rgb)), "read")
        return known, lo.view(np.float32), rgb
