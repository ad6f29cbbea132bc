"""GPU: sind_voc_transform_bow (the BowVector of ComputeBoW), the key-frame database sind_bowdb_* with the Python tails of DetectLoopCandidates /
DetectRelocalizationCandidates, and sind_match_by_bow_kf (ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*), src/ORBmatcher.cc:522-655) against the Python
restatement tests/loop_ref.py.  The reference cannot be built for the tests (DBoW2 needs OpenCV), so parity is against the restatement, as for every matcher
call.  All equalities: FP64 values and FP32 scores as bit patterns.  The "plenty of matches" guards are well under what the restatement finds on these scenes
(the found values stand beside them)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_STATE, SIND_E_CAPACITY = -1, -4, -5
COUNTS = ((0, 1, 63), (64, 65, 1500))                                            # B = 3, different n
bits64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)
bits32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)


def _kf_matcher(B, checkOri=True, nnratio=0.75, cap=4096):
    import match_scene as S
    from sindslam_amd.matcher import ORBmatcher
    return ORBmatcher(535.4, 539.2, 320.1, 247.6, 40.0, (0, 640, 0, 480), S._scale_factors(), nnratio=nnratio, checkOri=checkOri, cap=cap, max_batch=B)      # the camera is not read


@pytest.fixture(scope="module")
def bow_cases(stream):
    """(tree, 1500 descriptors, word and weight per descriptor from the restatement's descent), for the tiny tree and the stream vocabulary"""
    import bow_ref as W
    import bow_scene as B
    rng = np.random.default_rng(5)
    tiny = np.stack([B.bits(f) for f in list(B.TINY_EXPECT) + rng.integers(0, 257, 1500 - len(B.TINY_EXPECT)).tolist()])
    out = []
    for tree, d in ((B.tiny_tree(), tiny), (B.stream_vocabulary(stream), B.stream_frame(stream, 5)["desc"][:1500])):
        t = [W.transform_one(tree, f, 4) for f in d]
        out.append((tree, d, np.array([x[0] for x in t]), np.array([x[1] for x in t])))
    return out


@pytest.mark.parametrize("which", [0, 1])
def test_transform_bow_equals_the_restatement_at_every_count(bow_cases, which):
    import loop_ref as L
    from sindslam_amd.vocabulary import ORBVocabulary
    tree, desc, words, weights = bow_cases[which]
    assert len(desc) == 1500
    voc = ORBVocabulary(tree, cap=1500, max_batch=3)
    ref = {n: L.bow_vector_of(words[:n], weights[:n]) for c in COUNTS for n in c}
    for levelsup in (0, 4):
        for counts in COUNTS:
            frames = [desc[:n] for n in counts]
            got = voc.transform_bow(frames, levelsup)
            for n, (node, word, bw, bv), (rn, rw) in zip(counts, got, voc.transform(frames, levelsup)):
                assert np.array_equal(node, rn) and np.array_equal(word, rw) and np.array_equal(word, words[:n])
                assert bw.dtype == np.int32 and bv.dtype == np.float64 and np.array_equal(bw, ref[n][0]) and np.array_equal(bits64(bv), bits64(ref[n][1])), (levelsup, n)
    assert (weights == 0).sum() > 10 and len(ref[1500][0]) > (5 if which == 0 else 300)        # stopped words occur; found: 7 and 528 words
    assert len(ref[0][0]) == 0 and len(ref[1][0]) <= 1
    voc.close()


def test_transform_bow_adds_in_feature_order_and_leaves_stopped_frames_empty():
    import bow_ref as W
    import bow_scene as B
    import loop_ref as L
    import loop_scene as S
    from sindslam_amd.vocabulary import ORBVocabulary
    tree, desc = S.order_scene()
    rng = np.random.default_rng(9)
    long = np.stack([B.bits(f) for f in rng.choice([12, 45, 80, 130, 230, 21, 28, 33], 1500)])      # some two hundred additions of 0.1, 0.3, 0.7, ... per word
    voc = ORBVocabulary(tree, cap=1500, max_batch=3)
    frames = [desc, S.stopped_frame(), long]
    got = voc.transform_bow(frames, 4)
    for d, (node, word, bw, bv) in zip(frames, got):
        rw, rv = L.bow_vector(tree, d)
        assert np.array_equal(bw, rw) and np.array_equal(bits64(bv), bits64(rv))
    assert len(got[1][2]) == 0 and (got[1][0] == -1).all() and len(got[0][2]) == 5 and len(got[2][2]) == 6
    t = [W.transform_one(tree, f, 4) for f in desc]                              # the scene's claim: count * w gives other bits
    mult = {}
    for word, w, _, _ in t:
        if w > 0: mult[word] = mult.get(word, 0) + 1
    wt = {x[0]: x[1] for x in t}
    naive = np.array([mult[k] * wt[k] for k in sorted(mult)]); naive = naive / naive.sum()
    assert not np.array_equal(bits64(naive), bits64(got[0][3]))
    voc.close()


@pytest.mark.parametrize("n_live", [0, 1, 63, 64, 65])
def test_query_equals_the_restatement(n_live):
    import loop_ref as L
    import loop_scene as S
    from sindslam_amd.keyframe_db import KeyFrameDatabase
    main = S.query_vector(1, 900)
    rng = np.random.default_rng(n_live)
    queries = [main] + [S.random_vector(rng, rng.choice(main[0], k, replace=False)) for k in (0, 1, 64, 65)]
    cap, ops = S.database_history(n_live, main)
    db = KeyFrameDatabase(cap, cap_words=1024, max_queries=3)
    for op in ops:
        db.add(op[1], op[2]) if op[0] == "add" else db.erase(op[1])
    slots = S.apply_history(ops, cap)
    assert sum(s is not None for s in slots) == n_live and (n_live == 0 or None in slots)
    ref = [L.query(q, slots) for q in queries]
    if n_live >= 63:
        assert {0, 1, 64, 65, 900} <= set(ref[0][0].tolist()) and {0, 1, 64} <= set(ref[3][0].tolist()) and (ref[1][0] == 0).all()
        live = [s for s in range(cap) if slots[s] is not None]
        assert db.seq[live[1]] == db.seq.max() and (db.seq[[s for s in range(cap) if slots[s] is None]] == -1).all()      # added again: the last in the order of add
    for q, r in zip(queries, ref):                                               # Q = 1
        (common, first, score), = db.query([q])
        assert np.array_equal(common, r[0]) and np.array_equal(first, r[1]) and np.array_equal(bits32(score), bits32(r[2])), len(q[0])
    for (common, first, score), r in zip(db.query([queries[0], queries[1], queries[4]]), (ref[0], ref[1], ref[4])):      # Q = 3
        assert np.array_equal(common, r[0]) and np.array_equal(first, r[1]) and np.array_equal(bits32(score), bits32(r[2]))
    db.clear()
    (common, first, score), = db.query([main])
    assert (common == 0).all() and (first == -1).all() and (bits32(score) == 0).all() and (db.seq == -1).all()
    db.close()


def test_both_chains_on_a_stream_of_key_frames_equal_the_toy_reference(stream):
    import loop_scene as S
    from sindslam_amd.keyframe_db import KeyFrameDatabase
    from sindslam_amd.vocabulary import ORBVocabulary
    sc = S.kf_stream(stream)
    voc = ORBVocabulary(sc["tree"], cap=256, max_batch=8)
    frames = sc["desc"] + [sc["reloc"][t][0] for t in sorted(sc["reloc"])]
    refs = sc["bow"] + [sc["reloc"][t][1] for t in sorted(sc["reloc"])]
    bows = []
    for i in range(0, len(frames), 8):
        bows += [(bw, bv) for _, _, bw, bv in voc.transform_bow(frames[i:i + 8], 4)]
    for (bw, bv), (rw, rv) in zip(bows, refs):
        assert np.array_equal(bw, rw) and np.array_equal(bits64(bv), bits64(rv))
    db, toy = KeyFrameDatabase(S.N_KF, cap_words=256), S.Toy()
    res = S.drive_stream(sc, bows[:S.N_KF], dict(zip(sorted(sc["reloc"]), bows[S.N_KF:])), db, toy)
    for kind, t, got, ref in res:
        assert (bits32(got) == bits32(ref) if kind == "min_score" else got == ref), (kind, t)
    assert sum(len(r[3]) > 0 for r in res if r[0] == "loop" and r[1] >= S.LOOP_AT) >= 6 and all(len(r[3]) > 0 for r in res if r[0] == "reloc")
    db.close(); voc.close()


@pytest.mark.parametrize("ori", [True, False])
def test_search_by_bow_kf_on_stream_pairs_batched(stream, ori):
    import loop_ref as L
    import loop_scene as S
    pairs = [S.kf_stream_pair(stream, a, b, seed=b) for a, b in ((4, 5), (5, 6), (8, 9))]
    mt = _kf_matcher(3, ori)
    for (m, nm), (k1, k2) in zip(mt.SearchByBoWKF(pairs), pairs):
        mo, no, _ = L.search_by_bow_kf(k1, k2, 0.75, ori)
        assert nm == no and np.array_equal(m, mo)
        assert nm > 150                                                          # found: 313 / 316 / 331 with the orientation check, 321 / 334 / 353 without
    (m, nm), = mt.SearchByBoWKF(pairs[:1], nnratio=0.6)                          # the per-call ratio overrides the constructor's
    mo, no, _ = L.search_by_bow_kf(*pairs[0], 0.6, ori)
    assert nm == no and np.array_equal(m, mo)
    if not ori:
        _, _, choice = L.search_by_bow_kf(*pairs[1], 0.75, False)
        _, _, choice0 = L.search_by_bow_kf(*pairs[1], 0.75, False, sequential=False)
        assert (choice != choice0).sum() > 0                                     # found: 47 choices depend on vbMatched2
    mt.close()


def test_search_by_bow_kf_one_key_frame_against_three_candidates(stream):
    import loop_ref as L
    import loop_scene as S
    k1 = S.kf_stream_pair(stream, 9, 5, seed=0)[0]                               # LoopClosing::ComputeSim3: the current key frame on side 1 of every pair
    pairs = [(k1, S.kf_stream_pair(stream, 9, t, seed=t)[1]) for t in (6, 7, 8)]
    mt = _kf_matcher(3, True)
    for (m, nm), (a, b) in zip(mt.SearchByBoWKF(pairs), pairs):
        mo, no, _ = L.search_by_bow_kf(a, b, 0.75, True)
        assert nm == no and np.array_equal(m, mo) and nm > 130                   # found: about 270 / 320 / 340
    mt.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_search_by_bow_kf_contended_keypoints_validity_on_both_sides_and_every_node_size(seed):
    import loop_ref as L
    import loop_scene as S
    k1, k2 = S.kf_stress_pair(seed)
    none1 = {k: v[:0] for k, v in k1.items()}; none2 = {k: v[:0] for k, v in k2.items()}
    pairs = [(k1, k2), (none1, k2), (k1, none2), ({k: v[:65] for k, v in k1.items()}, k2)]
    for ori, least in ((True, 35), (False, 70)):                                 # found: 73 / 71 and 142 / 141
        mt = _kf_matcher(4, ori, cap=len(k2["node"]))                            # side 2 fills the capacity exactly
        got = mt.SearchByBoWKF(pairs)
        for (m, nm), (a, b) in zip(got, pairs):
            mo, no, choice = L.search_by_bow_kf(a, b, 0.75, ori)
            assert nm == no and np.array_equal(m, mo)
        assert got[0][1] > least and got[1][1] == 0 and len(got[1][0]) == 0 and got[2][1] == 0 and (got[2][0] == -1).all()
        mt.close()
    _, _, choice = L.search_by_bow_kf(k1, k2, 0.75, False)
    _, _, choice0 = L.search_by_bow_kf(k1, k2, 0.75, False, sequential=False)
    assert (choice != choice0).sum() > 120, "the scene is wrong, not the kernel"  # found: 254 / 269 choices depend on earlier claims
    assert (k2["valid"] == 0).sum() > 50 and (k1["valid"] == 0).sum() > 50


def test_search_by_bow_kf_bound_is_strictly_below_th_low():
    import loop_ref as L
    import loop_scene as S
    k1, k2 = S.th_low_pair()
    mo, no, _ = L.search_by_bow_kf(k1, k2, 0.75, False)
    ml, nl, _ = L.search_by_bow_kf(k1, k2, 0.75, False, strict=False)
    assert no == 3 and nl == 4 and not np.array_equal(mo, ml)                    # the scene tells '<' from '<='
    mt = _kf_matcher(1, False)
    (m, nm), = mt.SearchByBoWKF([(k1, k2)])
    assert nm == no and np.array_equal(m, mo)
    mt.close()


def test_transform_bow_errors_launch_nothing():
    import bow_scene as B
    from sindslam_amd import SindError
    from sindslam_amd._lib import lib
    from sindslam_amd.vocabulary import ORBVocabulary
    feats = np.stack([B.bits(f) for f in B.TINY_EXPECT]); big = np.concatenate([feats, feats, feats])
    voc = ORBVocabulary(B.tiny_tree(), cap=16, max_batch=2)
    with pytest.raises(SindError, match="capacity"):
        voc.transform_bow([big], 1)                                              # 21 descriptors > cap 16
    with pytest.raises(SindError, match="max_batch"):
        voc.transform_bow([feats, feats, feats], 1)
    node = np.full(32, 77, np.int32); word = np.full(32, 77, np.int32); bw = np.full(32, 77, np.int32); bv = np.full(32, 77.0); nw = np.full(3, 77, np.int32)
    p3 = lambda x: (C.c_void_p * 3)(x, x, x)
    def call(d, n, B_, bow_word=bw.ctypes.data):
        return lib().sind_voc_transform_bow(voc._h, p3(d), (C.c_int * 3)(n, n, n), B_, 1, (C.c_void_p * 3)(node.ctypes.data, None, None), (C.c_void_p * 3)(word.ctypes.data, None, None),
                                            (C.c_void_p * 3)(bow_word, bow_word, bow_word), p3(bv.ctypes.data), nw.ctypes.data_as(C.c_void_p))
    assert call(big.ctypes.data, 21, 1) == SIND_E_CAPACITY and call(feats.ctypes.data, 7, 3) == SIND_E_CAPACITY and call(None, 7, 1) == SIND_E_ARG
    assert call(feats.ctypes.data, 7, 1, bow_word=None) == SIND_E_ARG
    assert (node == 77).all() and (word == 77).all() and (bw == 77).all() and (bv == 77.0).all() and (nw == 77).all()
    assert call(None, 0, 2) == 0 and nw.tolist() == [0, 0, 77] and (bw == 77).all()        # empty frames are valid
    assert call(feats.ctypes.data, 7, 1) == 0 and nw[0] == 5 and bw[:5].tolist() == [0, 1, 2, 3, 5] and (bw[5:] == 77).all()      # 45 and 50 share word 1, 21 is stopped
    assert bv[:5].tolist() == [1.0 / 6.0, 2.0 / 6.0, 1.0 / 6.0, 1.0 / 6.0, 1.0 / 6.0] and (bv[5:] == 77.0).all() and node[:7].tolist() == [e[2] for e in B.TINY_EXPECT.values()]
    voc.close()
    wide = ORBVocabulary(B.tiny_tree(), cap=5000, max_batch=1)                   # the BowVector sorts a frame in LDS: 4096 descriptors at most, whatever cap says
    many = np.stack([B.bits(12)] * 4097)
    with pytest.raises(SindError, match="capacity"):
        wide.transform_bow([many], 1)
    (_, _, w1, v1), = wide.transform_bow([many[:4096]], 1)
    assert w1.tolist() == [5] and v1.tolist() == [1.0] and len(wide.transform([many], 1)[0][0]) == 4097
    wide.close()


def test_database_errors_launch_nothing():
    import loop_scene as S
    from sindslam_amd import SindError
    from sindslam_amd._lib import lib
    from sindslam_amd.keyframe_db import KeyFrameDatabase, _Query
    db = KeyFrameDatabase(4, cap_words=8, max_queries=2)
    v = S.flat([1, 4, 9])
    db.add(2, v)
    with pytest.raises(SindError, match="live"):
        db.add(2, v)
    with pytest.raises(SindError, match="capacity"):
        db.add(0, S.flat(range(9)))
    with pytest.raises(SindError, match="ascend"):
        db.add(0, (np.array([4, 1, 9], np.int32), v[1]))
    with pytest.raises(SindError, match="ascend"):
        db.add(0, (np.array([1, 4, 4], np.int32), v[1]))
    with pytest.raises(SindError, match="bad arguments"):
        db.add(4, v)
    with pytest.raises(SindError, match="max_queries"):
        db.query([v, v, v])
    assert db.seq.tolist() == [-1, -1, 0, -1]
    w = np.array([1, 4, 9], np.int32); bad = np.array([9, 4, 1], np.int32); x = v[1]
    add = lambda slot, word, value, n: lib().sind_bowdb_add(db._h, slot, C.c_void_p(word), C.c_void_p(value), n)
    assert add(2, w.ctypes.data, x.ctypes.data, 3) == SIND_E_STATE and add(0, w.ctypes.data, x.ctypes.data, 9) == SIND_E_CAPACITY and add(0, None, x.ctypes.data, 3) == SIND_E_ARG
    assert add(0, bad.ctypes.data, x.ctypes.data, 3) == SIND_E_ARG and add(-1, w.ctypes.data, x.ctypes.data, 3) == SIND_E_ARG
    common = np.full(4, 77, np.int32); first = np.full(4, 77, np.int32); score = np.full(4, 77, np.float32)
    def query(Q, word=w.ctypes.data, n=3, out=common.ctypes.data):
        arr = (_Query * 3)()
        for q in arr: q.n, q.word, q.value, q.common, q.first_word, q.score = n, word, x.ctypes.data, out, first.ctypes.data, score.ctypes.data
        return lib().sind_bowdb_query(db._h, arr, Q)
    assert query(3) == SIND_E_CAPACITY and query(1, word=None) == SIND_E_ARG and query(1, word=bad.ctypes.data) == SIND_E_ARG and query(1, n=9) == SIND_E_CAPACITY and query(1, out=None) == SIND_E_ARG
    assert (common == 77).all() and (first == 77).all() and (score == 77).all()
    assert query(1) == 0 and common.tolist() == [0, 0, 3, 0] and first.tolist() == [-1, -1, 1, -1] and score[2] == 1.0      # the handle still works, and the failed adds left no trace
    assert query(1, word=None, n=0) == 0 and common.tolist() == [0, 0, 0, 0]     # an empty query is valid
    db.erase(1); db.erase(2)                                                     # erasing a dead slot does nothing
    db.add(2, v); assert db.seq.tolist() == [-1, -1, 1, -1]
    db.close()


def test_search_by_bow_kf_errors_launch_nothing_and_leave_the_outputs():
    import loop_ref as L
    import loop_scene as S
    from sindslam_amd import SindError
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import _BowKF
    k1, k2 = S.kf_stress_pair(4)
    s1 = {k: v[:60] for k, v in k1.items()}; s2 = {k: v[:100] for k, v in k2.items()}
    mt = _kf_matcher(1, False, 0.75, cap=128)
    with pytest.raises(SindError, match="capacity"):
        mt.SearchByBoWKF([(k1, s2)])
    with pytest.raises(SindError, match="capacity"):
        mt.SearchByBoWKF([(s1, k2)])
    with pytest.raises(SindError, match="null array"):
        mt.SearchByBoWKF([(s1, dict(s2, valid=s2["valid"][:0]))])                # side 2 must say which keypoints hold a good map point
    with pytest.raises(SindError, match="node id"):
        mt.SearchByBoWKF([(s1, dict(s2, node=s2["node"] - 40))])
    with pytest.raises(SindError, match="bad arguments"):
        mt.SearchByBoWKF([(s1, s2)] * 2)                                         # B = 2 > max_batch 1
    u8, i32, f32 = (lambda a: np.ascontiguousarray(a, np.uint8)), (lambda a: np.ascontiguousarray(a, np.int32)), (lambda a: np.ascontiguousarray(a, np.float32))
    m = np.full(2000, 77, np.int32); nm = np.full(1, 77, np.int32)
    a = {}
    for s, k in (("1", k1), ("2", k2)): a.update({"node" + s: i32(k["node"]), "valid" + s: u8(k["valid"]), "angle" + s: f32(k["angle"]), "desc" + s: u8(k["desc"])})
    def call(n1, n2, B_=1, **null):
        q = _BowKF(n1=n1, n2=n2, match12=m.ctypes.data, nmatches=nm.ctypes.data, **{k: (None if k in null else v.ctypes.data) for k, v in a.items()})
        return lib().sind_match_by_bow_kf(mt._h, C.byref(q), B_, C.c_float(0.75), 0)
    assert call(129, 100) == SIND_E_CAPACITY and call(60, 129) == SIND_E_CAPACITY and call(60, 100, desc1=1) == SIND_E_ARG and call(60, 100, valid2=1) == SIND_E_ARG
    assert call(60, 100, valid1=1) == SIND_E_ARG and call(60, 100, B_=2) == SIND_E_ARG
    assert (m == 77).all() and nm[0] == 77
    assert call(0, 0, desc1=1, node2=1) == 0 and nm[0] == 0 and (m == 77).all()  # a count of 0 is valid, NULL arrays with it too
    (got, n), = mt.SearchByBoWKF([(s1, s2)])                                     # the handle still works
    mo, no, _ = L.search_by_bow_kf(s1, s2, 0.75, False)
    assert n == no and np.array_equal(got, mo)
    mt.close()
