"""KeyFrameDatabase — the reference's key-frame database (src/KeyFrameDatabase.cc:40-309) over the C ABI (include/sind_hip.h: sind_bowdb_*).  The BowVectors
live on the device and a query scores one vector against every stored key frame there (L1Scoring::score, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68);
the order-dependent list and graph logic of DetectLoopCandidates / DetectRelocalizationCandidates runs here on the host, on the query's three arrays.  The
two tails are plain functions of those arrays, so they can be checked without a device.  A key frame is a slot: the caller's index, 0 .. cap_slots - 1."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib

f32 = np.float32


class _Query(C.Structure):
    _fields_ = [("n", C.c_int), ("word", C.c_void_p), ("value", C.c_void_p), ("common", C.c_void_p), ("first_word", C.c_void_p), ("score", C.c_void_p)]


def sharing_words(common, first_word, seq, excluded=()):
    """lKFsSharingWords (:86-104, :207-222): the reference walks the query's words in ascending order and every word's list in push_back order, and appends a key
    frame where it first meets it -- at its smallest common word, behind the key frames added to the database before it: ordered by (first_word, sequence)."""
    ex = set(int(s) for s in excluded)
    return sorted((int(s) for s in np.nonzero(np.asarray(common) > 0)[0] if int(s) not in ex), key=lambda s: (int(first_word[s]), int(seq[s])))


def _min_common_words(common, sharing):
    max_common = max(int(common[s]) for s in sharing)
    return int(f32(max_common) * f32(0.8))                            # int minCommonWords = maxCommonWords*0.8f: an int-to-float product, truncated


def _retain(acc):
    """:175-196, :289-308: the entries above 0.75f * bestAccScore, a key frame once; acc: (best_acc, [(accScore, slot)])"""
    best_acc, entries = acc
    min_retain = f32(f32(0.75) * best_acc)
    out, seen = [], set()
    for a, s in entries:
        if a > min_retain and s not in seen:
            out.append(s); seen.add(s)
    return out


def loop_candidates_tail(common, first_word, score, seq, connected_slots, min_score, best_covisibles):
    """DetectLoopCandidates (:76-197) from a query's outputs.  connected_slots: pKF->GetConnectedKeyFrames() as slots (absent from the list and from the covisibility
    accumulation: mnLoopQuery is never set for them); best_covisibles: slot -> GetBestCovisibilityKeyFrames(10) as slots.  -> vpLoopCandidates as slots"""
    min_score = f32(min_score); connected = set(int(s) for s in connected_slots)
    sharing = sharing_words(common, first_word, seq, connected)
    if not sharing: return []
    min_common = _min_common_words(common, sharing)
    scored = [(f32(score[s]), s) for s in sharing if common[s] > min_common and f32(score[s]) >= min_score]
    if not scored: return []
    best_acc, entries = min_score, []
    for si, s in scored:
        best_score, acc, best = si, si, s
        for s2 in best_covisibles.get(s, ()):
            if s2 not in connected and common[s2] > 0 and common[s2] > min_common:       # mnLoopQuery == mnId && mnLoopWords > minCommonWords: scored in this query
                s2_score = f32(score[s2])
                acc = f32(acc + s2_score)
                if s2_score > best_score: best, best_score = s2, s2_score
        entries.append((acc, best))
        if acc > best_acc: best_acc = acc
    return _retain((best_acc, entries))


def reloc_candidates_tail(common, first_word, score, seq, reloc_score, best_covisibles):
    """DetectRelocalizationCandidates (:199-309) from a query's outputs.  reloc_score: f32 per slot, the persistent mRelocScore (0.0f at add); the entries of the slots
    scored here (common > minCommonWords) are overwritten, and a neighbour that shares a word but was not scored adds the value an earlier query left (:273-276).
    -> vpRelocCandidates as slots"""
    sharing = sharing_words(common, first_word, seq)
    if not sharing: return []
    min_common = _min_common_words(common, sharing)
    scored = []
    for s in sharing:
        if common[s] > min_common:
            reloc_score[s] = f32(score[s]); scored.append((f32(score[s]), s))
    if not scored: return []
    best_acc, entries = f32(0), []
    for si, s in scored:
        best_score, acc, best = si, si, s
        for s2 in best_covisibles.get(s, ()):
            if not common[s2] > 0: continue                            # mnRelocQuery != F->mnId
            s2_score = f32(reloc_score[s2])
            acc = f32(acc + s2_score)
            if s2_score > best_score: best, best_score = s2, s2_score
        entries.append((acc, best))
        if acc > best_acc: best_acc = acc
    return _retain((best_acc, entries))


class KeyFrameDatabase:
    """cap_slots key frames of at most cap_words words each, max_queries vectors per query call.  A BowVector is (bow_word i32, bow_value f64) as
    ORBVocabulary.transform_bow returns it."""

    def __init__(self, cap_slots, cap_words=4096, max_queries=1, device=0):
        h = C.c_void_p()
        check(lib().sind_bowdb_create(int(cap_slots), int(cap_words), int(max_queries), int(device), C.byref(h)), "sind_bowdb_create")
        self._h, self.cap_slots = h, int(cap_slots)
        lib().sind_bowdb_sequence.restype = C.c_longlong
        self.seq = np.full(cap_slots, -1, np.int64)                   # the order of add among the live slots
        self.reloc_score = np.zeros(cap_slots, np.float32)            # mRelocScore: 0.0f at add, overwritten when DetectRelocalizationCandidates scores the slot

    def close(self):
        if getattr(self, "_h", None):
            lib().sind_bowdb_destroy(self._h); self._h = None

    __del__ = close

    def add(self, slot, bow):
        word, value = np.ascontiguousarray(bow[0], np.int32), np.ascontiguousarray(bow[1], np.float64)
        if len(word) != len(value): raise ValueError("KeyFrameDatabase.add: words and values of different lengths")
        check(lib().sind_bowdb_add(self._h, int(slot), C.c_void_p(word.ctypes.data if word.size else None), C.c_void_p(value.ctypes.data if value.size else None), len(word)),
              "sind_bowdb_add")
        self.seq[slot] = lib().sind_bowdb_sequence(self._h, int(slot)); self.reloc_score[slot] = 0.0

    def erase(self, slot):
        check(lib().sind_bowdb_erase(self._h, int(slot)), "sind_bowdb_erase")
        self.seq[slot] = -1

    def clear(self):
        check(lib().sind_bowdb_clear(self._h), "sind_bowdb_clear")
        self.seq[:] = -1

    def query(self, bows):
        """bows: list of BowVectors -> list of (common i32 [cap_slots], first_word i32 [cap_slots], score f32 [cap_slots]); dead slots: 0, -1, 0.0"""
        Q = len(bows); arr = (_Query * Q)(); keep = []
        for q, (w, v) in zip(arr, bows):
            a = dict(word=np.ascontiguousarray(w, np.int32), value=np.ascontiguousarray(v, np.float64), common=np.zeros(self.cap_slots, np.int32),
                     first_word=np.full(self.cap_slots, -1, np.int32), score=np.zeros(self.cap_slots, np.float32))
            if len(a["word"]) != len(a["value"]): raise ValueError("KeyFrameDatabase.query: words and values of different lengths")
            q.n = len(a["word"])
            for k, x in a.items():
                setattr(q, k, x.ctypes.data if x.size else None)
            keep.append(a)
        check(lib().sind_bowdb_query(self._h, arr, Q), "sind_bowdb_query")
        return [(a["common"], a["first_word"], a["score"]) for a in keep]

    def DetectLoopCandidates(self, bow, connected_slots, min_score, best_covisibles):
        (common, first_word, score), = self.query([bow])
        return loop_candidates_tail(common, first_word, score, self.seq, connected_slots, min_score, best_covisibles)

    def DetectRelocalizationCandidates(self, bow, best_covisibles):
        (common, first_word, score), = self.query([bow])
        return reloc_candidates_tail(common, first_word, score, self.seq, self.reloc_score, best_covisibles)
