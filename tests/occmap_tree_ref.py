"""The snapshot tree's contract (include/sind_hip.h, "SNAPSHOT TREE"), restated literally in Python on top of tests/occmap_ref.py: a pointer tree built from
FlatMap.vox, octomap 1.9's prune() / pruneRecurs / pruneNode / isNodeCollapsible, updateInnerOccupancy (updateOccupancyChildren always, getAverageChildColor when
asked), writeData / writeNodesRecurs, the leaf walk and the .ot header, as recalled.  Independent of csrc/host/occmap_tree.hpp.  Beside the writer an .ot PARSER
(header + stream -> leaves) that shares nothing with it, so that a round trip proves something.  Parity with a real octomap build is unpinned; nothing here claims it."""
import struct

import numpy as np

import occmap_ref as R

F = np.float32
HEADER = "# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\nid ColorOcTree\nsize %d\nres %s\ndata\n"


class Node:
    __slots__ = ("v", "c", "ch")

    def __init__(self):
        self.v, self.c, self.ch = F(0), R.WHITE, None

    def has_children(self):
        return self.ch is not None and any(x is not None for x in self.ch)


def child_index(k, depth):
    b = 15 - depth
    return (((k[2] >> b) & 1) << 2) | (((k[1] >> b) & 1) << 1) | ((k[0] >> b) & 1)


class Tree:
    def __init__(self, flat, prune=True, inner_colour=False):
        """flat: occmap_ref.FlatMap.  prune, then updateInnerOccupancy (the other order gives the same tree: eight equal children average and maximise to themselves)"""
        self.P = flat.P; self.root = None; self.n_pruned = 0
        for k, (v, c) in flat.vox.items():
            if self.root is None:
                self.root = Node()
            n = self.root
            for d in range(16):
                if n.ch is None:
                    n.ch = [None] * 8
                i = child_index(k, d)
                if n.ch[i] is None:
                    n.ch[i] = Node()
                n = n.ch[i]
            n.v, n.c = F(v), tuple(int(x) for x in c)
        if prune:
            self.prune()
        if self.root is not None:
            self._update_inner(self.root, 0, inner_colour)

    # ---- OcTreeBaseImpl::prune
    @staticmethod
    def collapsible(n):
        if n.ch is None or n.ch[0] is None or n.ch[0].has_children():
            return False
        first = n.ch[0]
        for i in range(1, 8):
            c = n.ch[i]
            if c is None or c.has_children() or not (c.v == first.v and c.c == first.c):
                return False
        return True

    def _prune_node(self, n):
        if not self.collapsible(n):
            return False
        n.v, n.c, n.ch = n.ch[0].v, n.ch[0].c, None
        return True

    def _prune_recurs(self, n, depth, max_depth):
        if depth < max_depth:
            return sum(self._prune_recurs(c, depth + 1, max_depth) for c in (n.ch or ()) if c is not None)
        return int(self._prune_node(n))

    def prune(self):
        if self.root is None:
            return
        depth = 15
        while depth > 0:                                               # the root is never pruned
            num = self._prune_recurs(self.root, 0, depth)
            if num == 0:
                break
            self.n_pruned += num; depth -= 1

    # ---- updateInnerOccupancyRecurs
    def _update_inner(self, n, depth, colour):
        if not n.has_children():
            return
        kids = [c for c in n.ch if c is not None]
        for c in kids:
            self._update_inner(c, depth + 1, colour)
        n.v = max(c.v for c in kids)
        n.c = R.WHITE
        if colour:
            sel = [c.c for c in kids if c.c != R.WHITE]
            if sel:
                n.c = tuple(sum(c[j] for c in sel) // len(sel) for j in range(3))

    # ---- writeData, leaves, stats
    def walk(self):
        """pre-order: (node, depth, key of its lowest corner)"""
        if self.root is None:
            return
        stack = [(self.root, 0, (0, 0, 0))]
        while stack:
            n, d, k = stack.pop()
            yield n, d, k
            if n.ch is not None:
                s = 15 - d
                for i in range(7, -1, -1):
                    if n.ch[i] is not None:
                        stack.append((n.ch[i], d + 1, (k[0] | ((i & 1) << s), k[1] | (((i >> 1) & 1) << s), k[2] | (((i >> 2) & 1) << s))))

    def stream(self):
        out = bytearray()
        for n, _, _ in self.walk():
            mask = sum(1 << i for i in range(8) if n.ch is not None and n.ch[i] is not None)
            out += struct.pack("<f4B", float(n.v), n.c[0], n.c[1], n.c[2], mask)
        return bytes(out)

    def centre(self, k, d):
        s = 16 - d
        return F((float(((k >> s) << s) - 32768) + 0.5 * float(1 << s)) * self.P.res)

    def leaves(self, occupied_only=False):
        """[(x, y, z as float32, (r, g, b), depth)] in leaf_iterator order"""
        return [(self.centre(k[0], d), self.centre(k[1], d), self.centre(k[2], d), n.c, d) for n, d, k in self.walk()
                if not n.has_children() and (not occupied_only or n.v >= self.P.occ)]

    def leaf_nodes(self):
        """[(key of the lowest corner, depth, value, colour)] of every leaf"""
        return [(k, d, n.v, n.c) for n, d, k in self.walk() if not n.has_children()]

    def stats(self):
        st = dict(n_nodes=0, n_inner=0, n_leaves=0, n_pruned=self.n_pruned, n_occupied_leaves=0, leaves_at_depth=[0] * 17)
        for n, d, _ in self.walk():
            st["n_nodes"] += 1
            if n.has_children():
                st["n_inner"] += 1
            else:
                st["n_leaves"] += 1; st["leaves_at_depth"][d] += 1; st["n_occupied_leaves"] += bool(n.v >= self.P.occ)
        return st

    def ot(self):
        data = self.stream()
        return (HEADER % (len(data) // 8, "%g" % self.P.res)).encode() + data


def parse_ot(blob):
    """.ot bytes -> (id, size, res, leaves): leaves = [(key of the lowest corner, depth, value bits, (r, g, b))] in file order.  Written against the format's
    description (header lines up to `data`, then per node 4 + 3 + 1 bytes, children in ascending index after their parent), not against the writer above."""
    pos = blob.index(b"\ndata\n") + 6; head = blob[:pos].decode().split("\n")
    assert head[0] == "# Octomap OcTree file"
    fields = dict(line.split(" ", 1) for line in head if line and not line.startswith("#") and " " in line)
    size, res = int(fields["size"]), float(fields["res"]); body = blob[pos:]
    assert len(body) == 8 * size, (len(body), size)
    leaves = []; at = 0
    if size:
        pending = [(0, (0, 0, 0))]                                     # depth and corner of the nodes still to come, the next one last
        while pending:
            d, k = pending.pop()
            bits, r, g, b, mask = struct.unpack_from("<I4B", body, at); at += 8
            if mask == 0:
                leaves.append((k, d, bits, (r, g, b)))
            else:
                assert d < 16
                s = 15 - d
                pending.extend((d + 1, (k[0] + ((i & 1) << s), k[1] + ((i >> 1 & 1) << s), k[2] + ((i >> 2 & 1) << s))) for i in range(7, -1, -1) if mask >> i & 1)
    assert at == len(body)
    return fields["id"], size, res, leaves


def expand(leaves):
    """every leaf expanded to its finest voxels -> {key: (value bits, colour)}"""
    vox = {}
    for k, d, bits, c in leaves:
        n = 1 << (16 - d)
        for x in range(n):
            for y in range(n):
                for z in range(n):
                    vox[(k[0] + x, k[1] + y, k[2] + z)] = (bits, c)
    return vox
