"""The occupancy map's contract (include/sind_hip.h, "sind_occmap_*"), restated literally in Python: octomap 1.9's insertRay / computeRayKeys / updateNodeLogOdds /
integrateNodeColor as recalled, on a flat dict.  Independent of csrc/host/occmap.hpp: FP32 steps are numpy float32 scalars, FP64 steps Python floats, exp is math.exp.
Beside it PruneTree, a literal pointer octree WITH octomap's pruning (expand on update, prune on the way up, search returning the pruned leaf), which quantifies the
contract's second deliberate divergence.  Parity with a real octomap build is unpinned; nothing here claims it."""
import math

import numpy as np

F = np.float32
DBL_MAX = 1.7976931348623157e308
WHITE = (255, 255, 255)


class Params:
    def __init__(self, resolution=0.02, prob_hit=0.7, prob_miss=0.4, clamp_min=0.1192, clamp_max=0.971, occ_thres=0.7):
        lo = lambda p: F(math.log(p / (1 - p)))
        self.res = float(resolution); self.rf = 1.0 / self.res
        self.hit, self.miss, self.cmin, self.cmax, self.occ = lo(prob_hit), lo(prob_miss), lo(clamp_min), lo(clamp_max), lo(occ_thres)


def key(P, c):
    k = math.floor(P.rf * float(c)) + 32768
    return k if 0 <= k < 65536 else None


def key3(P, x, y, z):
    k = (key(P, x), key(P, y), key(P, z))
    return None if None in k else k


def coord(P, k):
    return (float(int(k) - 32768) + 0.5) * P.res


def ray(P, origin, end):
    """-> None (skipped) or (miss keys in order, end key, ended_by_length)"""
    o = [F(v) for v in origin]; e = [F(v) for v in end]
    ko, ke = key3(P, *o), key3(P, *e)
    if ko is None or ke is None:
        return None
    if ko == ke:
        return [], ke, False
    with np.errstate(all="ignore"):
        d = [e[i] - o[i] for i in range(3)]
        length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        d = [d[i] / length for i in range(3)]
    assert all(type(v) is F for v in d) and type(length) is F
    step, tmax, tdelta = [0] * 3, [DBL_MAX] * 3, [DBL_MAX] * 3
    for i in range(3):
        step[i] = 1 if d[i] > 0 else -1 if d[i] < 0 else 0
        if step[i]:
            border = coord(P, ko[i]) + float(F(step[i] * P.res * 0.5))
            tmax[i] = (border - float(o[i])) / float(d[i])
            tdelta[i] = P.res / abs(float(d[i]))
    cur = list(ko); misses = [ko]
    while True:
        dim = (0 if tmax[0] < tmax[2] else 2) if tmax[0] < tmax[1] else (1 if tmax[1] < tmax[2] else 2)
        cur[dim] += step[dim]; tmax[dim] += tdelta[dim]
        if not 0 <= cur[dim] < 65536:
            return misses, ke, True                                   # the guard of divergence 1 (a ray whose FP32 length underflowed)
        if tuple(cur) == ke:
            return misses, ke, False
        if min(tmax) > float(length):
            return misses, ke, True
        misses.append(tuple(cur))


def clamped_add(P, v, u):
    w = F(v) + F(u)
    return P.cmin if w < P.cmin else P.cmax if w > P.cmax else w


def blend(prev, new, p):
    return int(float(prev) * p + float(new) * (0.99 - p))


def probability(v):
    return 1. - (1. / (1. + math.exp(float(v))))


def finite(p):
    return bool(np.isfinite(p["x"]) and np.isfinite(p["y"]) and np.isfinite(p["z"]))


class FlatMap:
    """key -> [logodds, (r, g, b)]; every entry is a known voxel"""

    def __init__(self, P):
        self.P = P; self.vox = {}

    def update(self, k, u):
        v = self.vox.setdefault(k, [F(0), WHITE])
        v[0] = clamped_add(self.P, v[0], u)

    def colour(self, k, rgb):
        v = self.vox.get(k)
        if v is None:
            return False
        if v[1] != WHITE:
            p = probability(v[0]); rgb = tuple(blend(a, b, p) for a, b in zip(v[1], rgb))
        v[1] = tuple(int(c) for c in rgb)
        return True

    def insert(self, cloud, origin, sink=None):
        """one key frame -> stats.  sink, if given, receives the same update / colour calls (the pruning tree)."""
        P = self.P; st = dict(n_rays=0, n_skipped=0, n_coloured=0, n_miss_updates=0, n_new_voxels=0, n_ended_by_length=0); before = len(self.vox)
        for p in cloud:
            if not finite(p) or not p["z"] >= 0:
                continue
            r = ray(P, origin, (p["x"], p["y"], p["z"]))
            if r is None:
                st["n_skipped"] += 1; continue
            st["n_rays"] += 1; st["n_miss_updates"] += len(r[0]); st["n_ended_by_length"] += r[2]
            for k in r[0]:
                self.update(k, P.miss)
                if sink: sink.update(k, P.miss)
            self.update(r[1], P.hit)
            if sink: sink.update(r[1], P.hit)
        for p in cloud:
            if not finite(p):
                continue
            k = key3(P, p["x"], p["y"], p["z"])
            if k is None:
                continue
            rgb = (int(p["r"]), int(p["g"]), int(p["b"]))
            st["n_coloured"] += self.colour(k, rgb)
            if sink: sink.colour(k, rgb)
        st["n_new_voxels"] = len(self.vox) - before
        return st

    def occupied(self):
        """[(key, (r, g, b))] in leaf_iterator order: ascending Morton code from bit 15 down, z the most significant bit of each triple, then y, then x"""
        def morton(k):
            m = 0
            for b in range(15, -1, -1):
                m = (m << 3) | (((k[2] >> b) & 1) << 2) | (((k[1] >> b) & 1) << 1) | ((k[0] >> b) & 1)
            return m
        return [(k, self.vox[k][1]) for k in sorted((k for k, v in self.vox.items() if v[0] >= self.P.occ), key=morton)]


class _Node:
    __slots__ = ("v", "c", "ch")

    def __init__(self, v, c):
        self.v, self.c, self.ch = v, c, None


class PruneTree:
    """octomap's pointer tree, depth 16, with pruning.  n_pruned_colour counts the integrateNodeColor calls whose search ended on a pruned (coarser) leaf."""

    def __init__(self, P):
        self.P = P; self.root = None; self.n_pruned_colour = 0; self.n_prunes = 0

    @staticmethod
    def _pos(k, depth):
        b = 15 - depth
        return (((k[2] >> b) & 1) << 2) | (((k[1] >> b) & 1) << 1) | ((k[0] >> b) & 1)

    def update(self, k, u):
        created = self.root is None
        if created:
            self.root = _Node(F(0), WHITE)
        self._update(self.root, created, k, 0, u)

    def _update(self, node, just_created, k, depth, u):
        if depth == 16:
            node.v = clamped_add(self.P, node.v, u); return
        pos = self._pos(k, depth); created = False
        if node.ch is None or node.ch[pos] is None:
            if node.ch is None and not just_created:
                node.ch = [_Node(node.v, node.c) for _ in range(8)]    # a pruned leaf: expandNode copies it into eight children
            else:
                if node.ch is None:
                    node.ch = [None] * 8
                node.ch[pos] = _Node(F(0), WHITE); created = True
        self._update(node.ch[pos], created, k, depth + 1, u)
        c = node.ch
        if all(x is not None and x.ch is None for x in c) and all(x.v == c[0].v and x.c == c[0].c for x in c[1:]):
            node.v, node.c, node.ch = c[0].v, c[0].c, None; self.n_prunes += 1
        else:
            node.v = max(x.v for x in c if x is not None)

    def search(self, k):
        """-> (node, depth) of the leaf that holds k, or None"""
        node = self.root
        if node is None:
            return None
        for depth in range(16):
            if node.ch is None:
                return node, depth                                    # a pruned leaf: it stands for all 8 ** (16 - depth) voxels below it
            node = node.ch[self._pos(k, depth)]
            if node is None:
                return None
        return node, 16

    def colour(self, k, rgb):
        f = self.search(k)
        if f is None:
            return
        node, depth = f
        self.n_pruned_colour += depth < 16
        if node.c != WHITE:
            p = probability(node.v); rgb = tuple(blend(a, b, p) for a, b in zip(node.c, rgb))
        node.c = tuple(int(c) for c in rgb)

    def n_finest(self):
        def count(node, depth):
            if node is None:
                return 0
            return 8 ** (16 - depth) if node.ch is None else sum(count(x, depth + 1) for x in node.ch)
        return count(self.root, 0)
