"""ORBVocabulary — the reference's ComputeBoW (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259, BowVector.cpp:34-84) over the C ABI: transform gives the
feature vector, transform_bow the feature vector and the BowVector."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib


class _Tree(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("levels", C.c_int), ("child_start", C.c_void_p), ("child", C.c_void_p), ("desc", C.c_void_p), ("word_id", C.c_void_p),
                ("weight", C.c_void_p)]


class ORBVocabulary:
    """tree_arrays: dict with levels (m_L), child_start i32 [n_nodes + 1] / child i32 [n_nodes - 1] (CSR over m_nodes[i].children, node 0 = root),
    desc u8 [n_nodes, 32], word_id i32 [n_nodes] (-1 for inner nodes), weight f64 [n_nodes] (see include/sind_hip.h: sind_voc_tree).
    At most `cap` descriptors per frame and `max_batch` frames per transform."""

    def __init__(self, tree_arrays, cap=4096, max_batch=1, device=0):
        t = tree_arrays
        a = dict(child_start=np.ascontiguousarray(t["child_start"], np.int32), child=np.ascontiguousarray(t["child"], np.int32), desc=np.ascontiguousarray(t["desc"], np.uint8),
                 word_id=np.ascontiguousarray(t["word_id"], np.int32), weight=np.ascontiguousarray(t["weight"], np.float64))
        n = len(a["word_id"])
        if len(a["child_start"]) != n + 1 or len(a["child"]) != max(n - 1, 0) or a["desc"].shape != (n, 32) or len(a["weight"]) != n:
            raise ValueError("ORBVocabulary: tree arrays of inconsistent lengths")
        tree = _Tree(n, int(t["levels"]), *[a[k].ctypes.data if a[k].size else None for k in ("child_start", "child", "desc", "word_id", "weight")])
        h = C.c_void_p()
        check(lib().sind_voc_create(C.byref(tree), int(cap), int(max_batch), int(device), C.byref(h)), "sind_voc_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().sind_voc_destroy(self._h); self._h = None

    __del__ = close

    def transform(self, list_of_desc, levelsup=4):
        """list_of_desc: per frame u8 [n, 32] -> list of (node_id i32 [n], word_id i32 [n]); node_id -1 = not in the feature vector (stopped word)"""
        B = len(list_of_desc)
        desc = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in list_of_desc]
        node = [np.full(len(d), -1, np.int32) for d in desc]; word = [np.full(len(d), -1, np.int32) for d in desc]
        ptrs = lambda arrs: (C.c_void_p * B)(*[x.ctypes.data if x.size else None for x in arrs])
        n = (C.c_int * B)(*[len(d) for d in desc])
        check(lib().sind_voc_transform(self._h, ptrs(desc), n, B, int(levelsup), ptrs(node), ptrs(word)), "sind_voc_transform")
        return list(zip(node, word))

    def transform_bow(self, list_of_desc, levelsup=4):
        """list_of_desc: per frame u8 [n, 32] -> list of (node_id i32 [n], word_id i32 [n], bow_word i32 [n_words], bow_value f64 [n_words]): transform's two arrays
        and the frame's BowVector as std::map iterates it (TF_IDF, L1 norm; word ids ascending, values in the reference's order of FP64 operations)"""
        B = len(list_of_desc)
        desc = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in list_of_desc]
        node = [np.full(len(d), -1, np.int32) for d in desc]; word = [np.full(len(d), -1, np.int32) for d in desc]
        bw = [np.zeros(len(d), np.int32) for d in desc]; bv = [np.zeros(len(d), np.float64) for d in desc]
        ptrs = lambda arrs: (C.c_void_p * B)(*[x.ctypes.data if x.size else None for x in arrs])
        n = (C.c_int * B)(*[len(d) for d in desc]); nw = (C.c_int * B)()
        check(lib().sind_voc_transform_bow(self._h, ptrs(desc), n, B, int(levelsup), ptrs(node), ptrs(word), ptrs(bw), ptrs(bv), nw), "sind_voc_transform_bow")
        return [(node[b], word[b], bw[b][:nw[b]].copy(), bv[b][:nw[b]].copy()) for b in range(B)]
