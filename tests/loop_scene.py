"""Test scenes for the loop-closing front end (BowVector, key-frame database, SearchByBoW(KeyFrame, KeyFrame)), built on bow_scene.  A BowVector is
(words i32 ascending, values f64); a key frame of a search is a dict of per-keypoint arrays (see sindslam_amd/matcher.py)."""
import numpy as np

import bow_ref as W
import bow_scene as B
import loop_ref as L

f32, f64 = np.float32, np.float64


# ---- BowVector ----
def order_tree():
    """bow_scene.tiny_tree with weights whose repeated sums round: word 5 (node 9) weighs 0.1, and 0.1 added ten times is not 10 * 0.1"""
    tree = dict(B.tiny_tree())
    w = np.zeros(12); w[[2, 5, 6, 7, 8, 9, 11]] = [1.0 / 3.0, 0.3, 0.7, 0.2, 0.6, 0.1, 1.7]      # node 10 stays stopped
    tree["weight"] = w
    return tree


def order_scene():
    """(tree, desc): ten features on word 5 among features on five other words and on the stopped word, shuffled"""
    feats = [12] * 10 + [45] * 3 + [80] * 7 + [130] * 6 + [230] * 3 + [21] * 2
    rng = np.random.default_rng(7)
    return order_tree(), np.stack([B.bits(f) for f in rng.permutation(feats)])


def stopped_frame(n=5):
    """descriptors that all fall on tiny_tree's stopped word: an empty BowVector"""
    return np.stack([B.bits(21)] * n)


# ---- database vectors ----
def random_vector(rng, words):
    words = np.sort(np.asarray(words, np.int32))
    v = rng.uniform(0.05, 3.0, len(words)); v = v / v.sum() if len(v) else v
    return words, v.astype(np.float64)


def query_vector(seed, n):
    """n even word ids below 6000"""
    rng = np.random.default_rng(100 + seed)
    return random_vector(rng, 2 * rng.choice(3000, n, replace=False))


SHARES = (0, 1, 64, 65, "all")


def slot_vector(seed, q, share, extra=40):
    """a vector that shares `share` words with q (all of them for "all", at most len(q)), with other values, among `extra` odd word ids"""
    rng = np.random.default_rng(200 + seed)
    k = len(q[0]) if share == "all" else min(share, len(q[0]))
    mine = rng.choice(q[0], k, replace=False) if k else np.zeros(0, np.int32)
    return random_vector(rng, np.concatenate([mine, 2 * rng.choice(3000, extra, replace=False) + 1]))


def database_history(n_live, q, seed=0):
    """-> (cap_slots, ops): ops = ("add", slot, vector) / ("erase", slot) that leave n_live live slots with erased and never-used slots between them; slot k
    shares SHARES[k % 5] words with q.  Slot 1 (if it stays) is erased and added again with another vector, so it is the last in the order of add."""
    cap = n_live + n_live // 3 + 4
    rng = np.random.default_rng(300 + seed + n_live)
    slots = sorted(rng.choice(cap, min(cap, n_live + n_live // 4 + 1), replace=False).tolist())
    dead = set(slots[2::5][:len(slots) - n_live])
    ops = [("add", s, slot_vector(s, q, SHARES[s % 5])) for s in rng.permutation(slots).tolist()]
    ops += [("erase", s) for s in sorted(dead)]
    live = [s for s in slots if s not in dead]
    while len(live) > n_live: ops.append(("erase", live.pop()))
    if len(live) > 1: ops += [("erase", live[1]), ("add", live[1], slot_vector(1000 + live[1], q, 65))]
    return cap, ops


def apply_history(ops, cap):
    """-> the slots' vectors (None: dead) after ops"""
    slots = [None] * cap
    for op in ops: slots[op[1]] = op[2] if op[0] == "add" else None
    return slots


class HostDatabase:
    """the interface of sindslam_amd.keyframe_db.KeyFrameDatabase with the restatement's query (loop_ref.query) in the device's place: what feeds the Python
    tails in the CPU tests"""

    def __init__(self, cap_slots):
        self.slots = [None] * cap_slots; self.seq = np.full(cap_slots, -1, np.int64); self.reloc_score = np.zeros(cap_slots, np.float32); self.next = 0

    def add(self, slot, bow):
        assert self.slots[slot] is None
        self.slots[slot] = bow; self.seq[slot] = self.next; self.next += 1; self.reloc_score[slot] = 0.0

    def erase(self, slot):
        self.slots[slot] = None; self.seq[slot] = -1

    def clear(self):
        self.slots = [None] * len(self.slots); self.seq[:] = -1

    def query(self, bows):
        return [L.query(q, self.slots) for q in bows]

    def DetectLoopCandidates(self, bow, connected_slots, min_score, best_covisibles):
        from sindslam_amd.keyframe_db import loop_candidates_tail
        return loop_candidates_tail(*self.query([bow])[0], self.seq, connected_slots, min_score, best_covisibles)

    def DetectRelocalizationCandidates(self, bow, best_covisibles):
        from sindslam_amd.keyframe_db import reloc_candidates_tail
        return reloc_candidates_tail(*self.query([bow])[0], self.seq, self.reloc_score, best_covisibles)


class Toy:
    """loop_ref's object graph driven by slots: slot -> KeyFrame, the graph given as slots"""

    def __init__(self):
        self.db = L.KeyFrameDatabase(); self.kf = {}; self.ids = 0

    def add(self, slot, bow):
        self.kf[slot] = L.KeyFrame(slot, bow); self.db.add(self.kf[slot])       # a key frame added again is a new object: its members start afresh

    def erase(self, slot):
        self.db.erase(self.kf[slot])

    def clear(self):
        self.db.clear()

    def _graph(self, best_covisibles):
        for s, k in self.kf.items(): k.best_covisibles = [self.kf[c] for c in best_covisibles.get(s, ()) if c in self.kf]

    def _query(self, bow, connected=()):
        self.ids += 1
        q = L.KeyFrame(10000 + self.ids, bow); q.connected = {self.kf[c] for c in connected if c in self.kf}
        return q

    def DetectLoopCandidates(self, bow, connected_slots, min_score, best_covisibles):
        self._graph(best_covisibles)
        return [k.mnId for k in self.db.DetectLoopCandidates(self._query(bow, connected_slots), min_score)]

    def DetectRelocalizationCandidates(self, bow, best_covisibles):
        self._graph(best_covisibles)
        return [k.mnId for k in self.db.DetectRelocalizationCandidates(self._query(bow))]

    def sharing(self, bow, connected_slots=None):
        q = self._query(bow, connected_slots or ())
        return [k.mnId for k in (self.db.sharing_reloc(q) if connected_slots is None else self.db.sharing_loop(q))]


def flat(words):
    """equal weights 1 / n: two such vectors of n1 <= n2 words score common / n2"""
    words = np.sort(np.asarray(list(words), np.int32))
    return words, np.full(len(words), 1.0 / max(len(words), 1), np.float64)


# ---- a stream of key frames for the end-to-end test ----
N_KF, LOOP_AT = 40, 28
_stream = {}


def kf_stream(stream):
    """40 key frames along a path that comes back: key frame t looks at place t, from t = 28 on at place t - 26 again.  A place is a window of 150 descriptors
    into the pool the stream vocabulary was drawn from, 40 further per place, 80 % of them kept, a few bits flipped.  -> dict: tree, desc [t], bow [t] (the
    restatement's BowVectors), connected [t] (the three key frames before it in time) / covisibles [t] (three on either side, nearest first), reloc: {t: (desc, bow)} frames that
    look at the place of key frame t - 6 once more."""
    if "s" not in _stream:
        tree = B.stream_vocabulary(stream)
        pool = np.concatenate([B.stream_frame(stream, 3)["desc"], B.stream_frame(stream, 4)["desc"]])
        rng = np.random.default_rng(77)

        def look(place):
            idx = (place * 40 + np.nonzero(rng.random(150) < 0.8)[0]) % len(pool)
            d = pool[idx].copy()
            for i in range(len(d)):
                b = rng.integers(0, 256, 2); d[i, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
            return d

        def bow(d):
            return L.bow_vector(tree, d)

        place = [t if t < LOOP_AT else t - LOOP_AT + 2 for t in range(N_KF)]
        desc = [look(p) for p in place]
        near = [[c for c in range(t - 1, max(t - 4, -1), -1)] for t in range(N_KF)]
        both = [[c for d in (1, 2, 3) for c in (t - d, t + d) if 0 <= c < N_KF] for t in range(N_KF)]
        reloc = {}
        for t in (12, 25, 26, 39):
            d = look(place[t - 6]); reloc[t] = (d, bow(d))
        _stream["s"] = dict(tree=tree, desc=desc, bow=[bow(d) for d in desc], connected=near, covisibles=both, reloc=reloc, place=place)
    return _stream["s"]


def drive_stream(scene, bows, reloc_bows, db, toy):
    """The two chains over the stream, on `db` (KeyFrameDatabase or HostDatabase) and on the toy reference in step.  From key frame 8 on: minScore as
    LoopClosing::DetectLoop takes it (src/LoopClosing.cc:124-141: the lowest score among the connected key frames), DetectLoopCandidates, add.  Key frame 5 is
    culled at t = 15, key frame 3 erased and added again at t = 20; at four times a frame relocalises.  -> [(kind, t, got, expected)]"""
    out = []
    covis = {t: list(c) for t, c in enumerate(scene["covisibles"])}
    for t in range(N_KF):
        if t >= 8:
            connected = [c for c in scene["connected"][t] if c != 5 or t < 15]
            (_, _, score), = db.query([bows[t]])
            min_score = min([f32(1.0)] + [f32(score[c]) for c in connected])
            ref_min = min([f32(1.0)] + [f32(L.l1_score(bows[t], bows[c])[0]) for c in connected])
            out.append(("min_score", t, min_score, ref_min))
            out.append(("loop", t, db.DetectLoopCandidates(bows[t], connected, min_score, covis), toy.DetectLoopCandidates(bows[t], connected, ref_min, covis)))
        db.add(t, bows[t]); toy.add(t, bows[t])
        if t == 15: db.erase(5); toy.erase(5)
        if t == 20:
            db.erase(3); toy.erase(3); db.add(3, bows[3]); toy.add(3, bows[3])
        if t in reloc_bows:
            out.append(("reloc", t, db.DetectRelocalizationCandidates(reloc_bows[t], covis), toy.DetectRelocalizationCandidates(reloc_bows[t], covis)))
    return out


# ---- SearchByBoW(KeyFrame, KeyFrame) ----
def kf_stream_pair(stream, t1, t2, seed=0, drop=0.15):
    """frames t1 and t2 of the stream as two key frames, a share `drop` of either's keypoints without a good map point"""
    rng = np.random.default_rng(6000 + seed)
    out = []
    for t in (t1, t2):
        f = B.stream_frame(stream, t)
        out.append(dict(node=B.stream_nodes(stream, t), valid=((f["depth"] > 0) & (rng.random(len(f["octave"])) > drop)).astype(np.uint8), angle=f["angle"], desc=f["desc"]))
    return out[0], out[1]


def kf_stress_pair(seed):
    """bow_scene.bow_stress_pair (node sizes 0 / 1 / 63 / 64 / 65 / about 200 on either side, the contended node) with validity on side 2 as well; the three
    keypoints of the contended node stay valid"""
    k1, k2 = B.bow_stress_pair(seed)
    rng = np.random.default_rng(7000 + seed)
    k2 = dict(k2, valid=(rng.random(len(k2["node"])) > 0.12).astype(np.uint8))
    k2["valid"][k2["node"] == B.STRESS_CLAIMED_NODE] = 1
    return k1, k2


def th_low_pair():
    """One keypoint of side 1 per node, descriptors bits(k) so that distances are differences: node 3 has its best at exactly 50 and its second at 120 (the
    ratio test passes at 0.75: 50 < 90), node 4 at 49, node 5 at 51; node 6: the one at distance 50 is not valid, the next at 48 is; node 7: two keypoints of
    side 1 want the same keypoint at 50 and 49."""
    d1 = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 10), (7, 11)]
    d2 = [(3, 50), (3, 120), (4, 49), (4, 130), (5, 51), (5, 140), (6, 50), (6, 48), (6, 150), (7, 60), (7, 160)]
    mk = lambda d: dict(node=np.array([n for n, _ in d], np.int32), desc=np.stack([B.bits(k) for _, k in d]), angle=np.full(len(d), 30.0, np.float32), valid=np.ones(len(d), np.uint8))
    k1, k2 = mk(d1), mk(d2)
    k2["valid"][6] = 0
    return k1, k2
