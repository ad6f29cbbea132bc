"""CPU: the Python restatement of the loop-closing front end (tests/loop_ref.py) against known answers, the claims its scenes make, the Python tails of
sindslam_amd.keyframe_db against the toy object graph, and the public surface of the new calls (C header, Python classes) without a device."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def test_hand_computed_bow_vector_and_score_on_the_tiny_tree():
    import bow_scene as B
    import loop_ref as L
    tree = B.tiny_tree()                                                         # every weight 1, word 6 stopped
    v = L.bow_vector(tree, np.stack([B.bits(f) for f in (12, 45, 12, 21, 130)]))  # words 5, 1, 5, stopped, 0: values 2, 1, 1 over a norm of 4
    assert v[0].tolist() == [0, 1, 5] and v[1].tolist() == [0.25, 0.25, 0.5] and v[0].dtype == np.int32 and v[1].dtype == np.float64
    w = L.bow_vector(tree, np.stack([B.bits(f) for f in (80, 45)]))               # words 2, 1
    assert w[0].tolist() == [1, 2] and w[1].tolist() == [0.5, 0.5]
    score, common = L.l1_score(v, w)                                             # word 1: |0.25 - 0.5| - 0.25 - 0.5 = -0.5
    assert score == 0.25 and common == [1]
    e = L.bow_vector(tree, np.stack([B.bits(21)] * 3))
    assert len(e[0]) == 0 and len(e[1]) == 0                                     # only stopped words: the vector stays empty
    assert L.query(v, [w, None, v])[0].tolist() == [1, 0, 3] and L.query(v, [w, None, v])[1].tolist() == [1, -1, 0]


def test_score_of_a_vector_with_itself_is_one_and_of_disjoint_vectors_zero(stream):
    import loop_ref as L
    import loop_scene as S
    for n in (1, 64, 900):
        v = S.query_vector(n, n)
        s, common = L.l1_score(v, v)
        assert abs(s - 1.0) <= np.spacing(f64(1.0)) and len(common) == n
        d = S.slot_vector(n, v, 0)
        s0, c0 = L.l1_score(v, d)
        assert s0 == 0.0 and c0 == [] and L.l1_score(d, v)[0] == 0.0
    assert L.l1_score(S.flat([]), S.flat([3]))[0] == 0.0


def test_summation_order_matters_on_the_scenes(stream):
    """without this the GPU test could not tell a kernel that multiplies, or reduces the norm as a tree, from a right one"""
    import bow_ref as W
    import loop_ref as L
    import loop_scene as S
    tree, desc = S.order_scene()
    t = [W.transform_one(tree, f, 4) for f in desc]
    words, weights = np.array([x[0] for x in t]), np.array([x[1] for x in t])
    assert (words == 5).sum() == 10 and weights[words == 5].tolist() == [0.1] * 10
    rep = f64(0.1)
    for _ in range(9): rep = f64(rep + f64(0.1))
    assert rep != f64(10) * f64(0.1)                                             # w + w + ... is not count * w
    bw, bv = L.bow_vector_of(words, weights)
    raw = {k: (weights[words == k][0], (words == k).sum()) for k in bw.tolist()}
    norm_rep = f64(0)
    for k in bw.tolist():
        s = f64(raw[k][0])
        for _ in range(raw[k][1] - 1): s = f64(s + raw[k][0])
        norm_rep = f64(norm_rep + s)
        if k == 5: assert s == rep
    assert any(f64(raw[k][0]) * raw[k][1] != _repeat(raw[k][0], raw[k][1]) for k in bw.tolist())
    assert bv[bw.tolist().index(5)] == f64(rep / norm_rep)
    # the ordered norm against numpy's pairwise sum, on the stream scene's larger vectors
    sc = S.kf_stream(stream)
    differs = 0
    for d in sc["desc"][:6]:
        t = [W.transform_one(sc["tree"], f, 4) for f in d]
        v = {}
        for word, w, _, _ in t:
            if w > 0: v[word] = f64(v[word] + w) if word in v else f64(w)
        vals = np.array([v[k] for k in sorted(v)], np.float64)
        ordered = f64(0)
        for x in vals: ordered = f64(ordered + np.fabs(x))
        differs += ordered != np.sum(vals)
    assert differs > 0


def _repeat(w, count):
    s = f64(w)
    for _ in range(count - 1): s = f64(s + f64(w))
    return s


@pytest.mark.parametrize("seed", range(6))
def test_sharing_list_is_ordered_by_first_word_and_add_sequence(seed):
    """random add / erase / re-add histories over a small vocabulary: sorting by (first_word, add sequence) gives lKFsSharingWords as the per-word lists give it"""
    import loop_ref as L
    import loop_scene as S
    from sindslam_amd.keyframe_db import sharing_words
    rng = np.random.default_rng(seed)
    cap = 24
    db, toy = S.HostDatabase(cap), S.Toy()
    vec = lambda: S.random_vector(rng, rng.choice(30, rng.integers(1, 9), replace=False))
    checked = 0
    for step in range(120):
        s = int(rng.integers(0, cap))
        if db.slots[s] is None:
            v = vec(); db.add(s, v); toy.add(s, v)
        elif rng.random() < 0.6:
            db.erase(s); toy.erase(s)
        if step % 5 == 4:
            q = vec()
            common, first, _ = L.query(q, db.slots)
            assert sharing_words(common, first, db.seq) == toy.sharing(q)
            connected = [int(c) for c in rng.choice(cap, 6, replace=False)]
            got = sharing_words(common, first, db.seq, connected)
            assert got == toy.sharing(q, connected) and not set(got) & set(connected)
            checked += len(got) > 3
    assert checked > 5
    db.clear(); toy.clear()
    assert sharing_words(*L.query(vec(), db.slots)[:2], db.seq) == toy.sharing(vec()) == []


def _both(cap=8):
    import loop_scene as S
    return S.HostDatabase(cap), S.Toy()


def test_tails_on_an_empty_database_no_shared_word_and_low_scores():
    import loop_scene as S
    db, toy = _both()
    q = S.flat(range(10))
    for d in (db, toy):
        assert d.DetectLoopCandidates(q, [], 0.0, {}) == [] and d.DetectRelocalizationCandidates(q, {}) == []
    for d in (db, toy):
        d.add(0, S.flat(range(100, 110))); d.add(1, S.flat(range(200, 210)))
        assert d.DetectLoopCandidates(q, [], 0.0, {}) == [] and d.DetectRelocalizationCandidates(q, {}) == []        # no shared word
        d.add(2, S.flat(range(0, 10))); d.add(3, S.flat(list(range(0, 9)) + [300]))
        assert d.DetectLoopCandidates(q, [], 1.5, {2: [3], 3: [2]}) == []                                              # every score under min_score
        assert d.DetectLoopCandidates(q, [], 1.0, {}) == [2]                                                           # si >= minScore, not >
        assert d.DetectLoopCandidates(q, [2], 0.5, {3: [2]}) == [3]                                                    # a connected key frame: not listed, not accumulated
        assert d.DetectLoopCandidates(q, [], 0.5, {}) == [2, 3] and d.DetectRelocalizationCandidates(q, {}) == [2, 3]


def test_tails_best_covisible_replaces_and_a_duplicate_is_removed():
    import loop_scene as S
    q = S.flat(range(10))
    for d in _both():
        d.add(4, S.flat(list(range(0, 9)) + [300]))                              # 9 common words, score 0.9; listed first (added first)
        d.add(1, S.flat(range(0, 10)))                                           # score 1
        d.add(6, S.flat(range(0, 5)))                                            # 5 common words: not above minCommonWords = 8
        assert d.DetectLoopCandidates(q, [], 0.1, {}) == [4, 1]
        assert d.DetectLoopCandidates(q, [], 0.1, {4: [1, 6]}) == [1]            # 4's entry is led by its neighbour 1 (1.9), 1's own entry (1.0) falls under 0.75 * 1.9
        assert d.DetectLoopCandidates(q, [], 0.1, {4: [1], 1: [4]}) == [1]       # both entries name 1: once
        assert d.DetectRelocalizationCandidates(q, {4: [1], 1: [4]}) == [1]
        assert d.DetectRelocalizationCandidates(q, {4: [6]}) == [4, 1]           # 6 shares words but was never scored: adds 0


def test_relocalisation_adds_the_score_an_earlier_query_left():
    import loop_scene as S
    for d in _both():
        d.add(0, S.flat(range(0, 10))); d.add(1, S.flat(range(20, 30)))
        covis = {1: [0]}
        f2 = S.flat(list(range(20, 30)) + [0])                                   # 10 words of key frame 1, one of key frame 0: 0 shares a word and is not scored
        assert d.DetectRelocalizationCandidates(f2, covis) == [1]                # reloc_score of 0 is still 0.0f
        assert d.DetectRelocalizationCandidates(S.flat(range(0, 10)), covis) == [0]      # scores key frame 0: 1.0
        assert d.DetectRelocalizationCandidates(f2, covis) == [0]                # now 0's stale 1.0 beats 1's own 10 / 11 and leads the entry
        d.erase(0); d.add(0, S.flat(range(0, 10)))
        assert d.DetectRelocalizationCandidates(f2, covis) == [1]                # added again: 0.0f again


def test_tails_equal_the_toy_reference_on_the_key_frame_stream(stream):
    import loop_scene as S
    sc = S.kf_stream(stream)
    db, toy = S.HostDatabase(S.N_KF), S.Toy()
    res = S.drive_stream(sc, sc["bow"], {t: b for t, (_, b) in sc["reloc"].items()}, db, toy)
    for kind, t, got, ref in res:
        assert got == ref, (kind, t)
    loops = [r for r in res if r[0] == "loop"]
    assert sum(len(r[3]) > 0 for r in loops if r[1] >= S.LOOP_AT) >= 6 and all(len(r[3]) > 0 for r in res if r[0] == "reloc")
    assert any(r[3] and 3 in r[3] for r in loops) or any(3 in r[3] for r in res if r[0] == "reloc")      # the key frame added again is found


def test_the_strict_bound_is_pinned_by_the_scene():
    import loop_ref as L
    import loop_scene as S
    k1, k2 = S.th_low_pair()
    m, n, _ = L.search_by_bow_kf(k1, k2, 0.75, False)
    m_le, n_le, _ = L.search_by_bow_kf(k1, k2, 0.75, False, strict=False)
    assert m.tolist() == [-1, 2, -1, 7, -1, 9] and n == 3                        # 50: no, 49: yes, 51: no, the invalid one skipped, 50 then 49 on the same keypoint
    assert m_le.tolist() == [0, 2, -1, 7, 9, -1] and n_le == 4


def test_kf_search_scenes_exercise_validity_and_claims(stream):
    import bow_scene as B
    import loop_ref as L
    import loop_scene as S
    k1, k2 = S.kf_stress_pair(1)
    m, n, choice = L.search_by_bow_kf(k1, k2, 0.75, False)
    _, _, choice0 = L.search_by_bow_kf(k1, k2, 0.75, False, sequential=False)
    assert n == (m >= 0).sum() and n > 40 and (choice != choice0).sum() > 0
    taken = m[m >= 0]
    assert len(set(taken.tolist())) == len(taken) and k2["valid"][taken].all() and k1["valid"][m >= 0].all()
    assert (k2["valid"] == 0).sum() > 50 and (k1["valid"] == 0).sum() > 50
    mo, no, _ = L.search_by_bow_kf(k1, k2, 0.75, True)
    assert no == (mo >= 0).sum() <= n and ((mo == m) | (mo == -1)).all()
    a, b = S.kf_stream_pair(stream, 5, 6, seed=6)
    m, n, _ = L.search_by_bow_kf(a, b, 0.75, True)
    assert n == (m >= 0).sum() and n > 100


def test_public_header_declares_the_new_calls_as_c(tmp_path):
    src = tmp_path / "surface.c"
    src.write_text('#include "sind_hip.h"\n'
                   "int (*const transform_bow)(sind_voc*, const uint8_t* const*, const int*, int, int, int* const*, int* const*, int* const*, double* const*, int*) = &sind_voc_transform_bow;\n"
                   "int (*const db_create)(int, int, int, int, sind_bowdb**) = &sind_bowdb_create;\n"
                   "int (*const db_destroy)(sind_bowdb*) = &sind_bowdb_destroy;\n"
                   "int (*const db_add)(sind_bowdb*, int, const int*, const double*, int) = &sind_bowdb_add;\n"
                   "int (*const db_erase)(sind_bowdb*, int) = &sind_bowdb_erase;\n"
                   "int (*const db_clear)(sind_bowdb*) = &sind_bowdb_clear;\n"
                   "int (*const db_query)(sind_bowdb*, const sind_bowdb_query_item*, int) = &sind_bowdb_query;\n"
                   "int (*const by_bow_kf)(sind_match*, const sind_match_bow_kf*, int, float, int) = &sind_match_by_bow_kf;\n"
                   "int main(void) { return (int)(sizeof(sind_bowdb_query_item) + sizeof(sind_match_bow_kf)); }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_classes_have_the_new_methods():
    from sindslam_amd.keyframe_db import KeyFrameDatabase                         # importing the modules loads no library
    from sindslam_amd.matcher import ORBmatcher
    from sindslam_amd.vocabulary import ORBVocabulary
    assert callable(ORBVocabulary.transform_bow) and callable(ORBmatcher.SearchByBoWKF)
    for name in ("add", "erase", "clear", "query", "DetectLoopCandidates", "DetectRelocalizationCandidates"):
        assert callable(getattr(KeyFrameDatabase, name))


def test_the_library_exports_the_new_symbols():
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "sindslam_amd", "libsind_hip.so")], text=True)
    for sym in ("sind_voc_transform_bow", "sind_bowdb_create", "sind_bowdb_destroy", "sind_bowdb_add", "sind_bowdb_erase", "sind_bowdb_clear", "sind_bowdb_query",
                "sind_bowdb_sequence", "sind_match_by_bow_kf"):
        assert f" T {sym}\n" in out, sym
