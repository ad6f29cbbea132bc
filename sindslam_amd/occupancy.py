"""Occupancy map of the mapping consumer — Python mirror of the octree part of the reference's key-frame callback (octomap_pub/src/pubPointCloud.cc:299-365:
insertRay per point, integrateNodeColor per point, the walk over the occupied leaves) over the C ABI (sind_occmap_*, contract in include/sind_hip.h).  The contract is
restated from octomap 1.9 as recalled; parity with a real octomap build is unpinned.  The map is flat (depth 16 only); octomap's inner nodes, prune(), the .ot file, fullMapToMsg and the leaf
walk come from a snapshot tree taken from it (tree, leaves, write_ot, full_map_msg, size_nodes)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import SindError, check, lib, ptr
from .cloud import POINT_DTYPE, _host_lib, _pack

OCC_STATS_DTYPE = np.dtype([("n_rays", "i4"), ("n_skipped", "i4"), ("n_coloured", "i4"), ("n_miss_updates", "i4"), ("n_new_voxels", "i4")])
TREE_STATS_DTYPE = np.dtype([("n_nodes", "i4"), ("n_inner", "i4"), ("n_leaves", "i4"), ("n_pruned", "i4"), ("n_occupied_leaves", "i4"), ("leaves_at_depth", "i4", (17,))])
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
        """the number of known voxels (not octomap's size(), which counts inner nodes: that is size_nodes())"""
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

    # ---- the snapshot tree: octomap's inner nodes, prune(), writeData, .ot and leaf iteration over the flat map (contract in include/sind_hip.h, "SNAPSHOT TREE";
    # restated from octomap 1.9 as recalled, parity with a real octomap build unpinned).  Read-only on the map.  Pruning is a bottom-up sweep over levels, which on a
    # tree that starts flat gives what OcTreeBaseImpl::prune()'s loop over depths gives.

    def _tree(self, prune, inner_colour, occupied_only, want_data, want_leaves):
        st = np.zeros(1, TREE_STATS_DTYPE); n = np.zeros(1, np.int32); f = self._f("tree"); flags = (int(bool(prune)), int(bool(inner_colour)), int(bool(occupied_only)))
        self._check(f(self._h, *flags, None, C.c_size_t(0), None, None, 0, ptr(n), ptr(st)), "tree")
        data = np.zeros(8 * int(st[0]["n_nodes"]) if want_data else 0, np.uint8); nl = int(n[0]) if want_leaves else 0
        leaves = np.zeros(nl, POINT_DTYPE); depth = np.zeros(nl, np.uint8)
        if len(data) or nl:
            self._check(f(self._h, *flags, ptr(data) if len(data) else None, C.c_size_t(len(data)), ptr(leaves) if nl else None, ptr(depth) if nl else None, nl, ptr(n),
                          ptr(st)), "tree")
        return st[0].copy(), data, leaves, depth

    def tree(self, prune=True, inner_colour=False, occupied_only=False):
        """-> dict(stats (TREE_STATS_DTYPE: n_nodes is octomap's size()), data (writeData's stream: 8 bytes per node in pre-order, uint8 [8 n_nodes]), leaves
        (POINT_DTYPE: centre and colour, leaf_iterator order), depth (uint8 per leaf)).  inner_colour=False leaves inner nodes white, as the reference's tree has them
        (it never calls updateInnerOccupancy); True gives them getAverageChildColor, bottom-up."""
        st, data, leaves, depth = self._tree(prune, inner_colour, occupied_only, True, True)
        return dict(stats=st, data=data, leaves=leaves, depth=depth)

    def leaves(self, prune=True, occupied_only=True):
        """-> (leaves, depth).  The defaults give the list the reference's loop over the tree walks (:349-365); prune=False, occupied_only=True equals occupied()."""
        _, _, leaves, depth = self._tree(prune, False, occupied_only, False, True)
        return leaves, depth

    def size_nodes(self, prune=True):
        """octomap's size(): inner nodes and leaves of the (pruned) tree"""
        return int(self._tree(prune, False, False, False, False)[0]["n_nodes"])

    def write_ot(self, path, prune=True, inner_colour=False):
        """octotree->write(path): the .ot header and the stream"""
        self._check(self._f("write_ot")(self._h, int(bool(prune)), int(bool(inner_colour)), os.fsencode(path)), "write_ot")

    def full_map_msg(self, prune=True, inner_colour=False):
        """octomap_msgs::fullMapToMsg as a dict: id, resolution, binary, data (bytes)"""
        return dict(id="ColorOcTree", resolution=self.resolution, binary=False, data=self._tree(prune, inner_colour, False, True, False)[1].tobytes())

    def read(self, keys):
        """keys [n, 3] uint16 -> known [n] u1, logodds [n] f4, rgb [n, 3] u1 (zeros where unknown)"""
        k = np.ascontiguousarray(keys, np.uint16).reshape(-1, 3); n = len(k)
        known = np.zeros(n, np.uint8); lo = np.zeros(n, np.uint32); rgb = np.zeros((n, 3), np.uint8)
        self._check(self._f("read")(self._h, ptr(k), n, ptr(known), ptr(lo), ptr(rgb)), "read")
        return known, lo.view(np.float32), rgb
