"""CPU: the Python restatement of the vocabulary-guided matching (tests/bow_ref.py) against properties nothing else pins, the scenes' own claims, and
the public surface of the new calls (C header, Python classes) without a device."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def stream_pair(stream):
    import bow_scene as B
    return B.bow_pair(stream, 5, 6, seed=6)


@pytest.fixture(scope="module")
def stress_pair():
    import bow_scene as B
    return B.bow_stress_pair(1)


def _check_bow_matches(kf, cur, nnratio, choice):
    """every key-frame keypoint that matched took, among its node's frame keypoints no earlier entry holds, the first of the nearest, within TH_LOW, and passed the ratio test"""
    import bow_ref as W
    fv_f = W.feature_vector(cur["node"])
    taken = choice[choice >= 0]
    assert len(set(taken.tolist())) == len(taken)                              # no frame keypoint is matched twice
    owner = np.full(len(cur["node"]), -1, np.int64); owner[taken] = np.nonzero(choice >= 0)[0]
    for ikf in np.nonzero(choice >= 0)[0]:
        i_f = choice[ikf]
        assert kf["valid"][ikf] and kf["node"][ikf] == cur["node"][i_f] >= 0
        free = [j for j in fv_f[int(kf["node"][ikf])] if owner[j] < 0 or owner[j] >= ikf]       # entries act in ascending key-frame index
        d = [W.hamming(kf["desc"][ikf], cur["desc"][j]) for j in free]
        assert free[int(np.argmin(d))] == i_f                                   # argmin: the first of equal minima
        s = sorted(d); best1, best2 = s[0], (s[1] if len(s) > 1 else 256)
        assert best1 <= W.TH_LOW and f32(best1) < f32(f32(nnratio) * f32(best2))
    return len(taken)


@pytest.mark.parametrize("nnratio", [0.7, 0.75])
def test_every_bow_match_shares_a_node_is_near_passes_the_ratio_test_and_is_unique(stream_pair, stress_pair, nnratio):
    import bow_ref as W
    for kf, cur in (stream_pair, stress_pair):
        m, nm, choice = W.search_by_bow(kf, cur, nnratio, check_orientation=False)
        assert _check_bow_matches(kf, cur, nnratio, choice) == nm == (m >= 0).sum()
        assert np.array_equal(np.sort(m[m >= 0]), np.nonzero(choice >= 0)[0])
        mo, nmo, _ = W.search_by_bow(kf, cur, nnratio, check_orientation=True)
        assert nmo == (mo >= 0).sum() <= nm and ((mo == m) | (mo == -1)).all()   # the orientation check only removes
    assert nm > {0.7: 54, 0.75: 67}[nnratio]                                    # stress scene, found: 108 / 134


def test_stress_scene_exercises_the_claims_and_every_node_size():
    import bow_ref as W
    import bow_scene as B
    for seed, least in ((1, 92), (2, 104)):                                    # found: 185 / 209 choices differ once the claims are ignored
        kf, cur = B.bow_stress_pair(seed)
        m, _, choice = W.search_by_bow(kf, cur, 0.7, check_orientation=False)
        _, _, choice0 = W.search_by_bow(kf, cur, 0.7, check_orientation=False, sequential=False)
        assert (choice != choice0).sum() >= least
        for side in (kf, cur):
            sizes = np.bincount(side["node"][side["node"] >= 0])
            assert {1, 63, 64, 65} <= set(sizes.tolist()) and (sizes >= 190).sum() >= 2 and (side["node"] == -1).sum() > 30
        nk, nc = set(kf["node"].tolist()), set(cur["node"].tolist())
        assert nk - nc - {-1} and nc - nk - {-1}                                # nodes on one side only
        held = cur["node"] == B.STRESS_CLAIMED_NODE
        assert held.sum() == 3 and (m[held] >= 0).all() and (kf["node"] == B.STRESS_CLAIMED_NODE).sum() == 40       # all of a node's frame keypoints claimed


def _tri_scenes(stream):
    import bow_scene as B
    return [B.tri_stream_pair(stream, 5, 6, seed=6), B.tri_special_pair(0)]


@pytest.mark.parametrize("only_stereo", [0, 1])
def test_triangulation_loop_is_the_minimum_distance_last_on_ties_over_the_static_candidates(stream, only_stereo):
    import bow_ref as W
    found = []
    for cam, sc, T2, Cw1, F12, k1, k2 in _tri_scenes(stream):
        m12, nm, pairs = W.search_for_triangulation(cam, sc, T2, Cw1, F12, k1, k2, only_stereo, check_orientation=False)
        epi = W.epipole(cam, T2, Cw1); fv2 = W.feature_vector(k2["node"])
        expect = np.full(len(k1["node"]), -1, np.int32)
        for i1 in range(len(k1["node"])):
            if k1["node"][i1] < 0 or k1["has_mp"][i1] or (only_stereo and not k1["u_right"][i1] >= 0): continue
            line = W.epipolar_line(k1["un_xy"][i1], F12)
            cand = [(W.tri_candidate_ok(k1, k2, i1, i2, line, epi, sc, only_stereo), i2) for i2 in fv2.get(int(k1["node"][i1]), [])]
            cand = [(d, -i2) for d, i2 in cand if d is not None]
            if cand: expect[i1] = -min(cand)[1]
        assert np.array_equal(m12, expect) and nm == (m12 >= 0).sum() == len(pairs)
        assert pairs == [(i, int(m12[i])) for i in np.nonzero(m12 >= 0)[0]]
        mo, nmo, po = W.search_for_triangulation(cam, sc, T2, Cw1, F12, k1, k2, only_stereo, check_orientation=True)
        assert nmo == (mo >= 0).sum() == len(po) <= nm and ((mo == m12) | (mo == -1)).all()
        found.append(nm)
    assert found[0] > (70 if only_stereo else 145) and found[1] > (34 if only_stereo else 97)      # found: 291 / 195 and 140 / 68


def test_special_triangulation_scene_has_the_tie_the_epipole_and_the_zero_denominator():
    import bow_ref as W
    import bow_scene as B
    cam, sc, T2, Cw1, F12, k1, k2 = B.tri_special_pair(0)
    m12, _, _ = W.search_for_triangulation(cam, sc, T2, Cw1, F12, k1, k2, 0, check_orientation=False)
    n = len(k1["node"])
    assert np.array_equal(m12[:20], np.arange(20) + n + 20)                      # three identical candidates each: the last one wins
    for i in range(20):
        assert (k2["desc"][i] == k2["desc"][n + i]).all() and (k2["desc"][i] == k2["desc"][n + 20 + i]).all()
    ex, ey = W.epipole(cam, T2, Cw1)
    assert k2["un_xy"][20, 0] == ex and k2["un_xy"][20, 1] == ey and k1["u_right"][20] < 0 and k2["u_right"][20] < 0
    assert (k1["desc"][20] == k2["desc"][20]).all() and m12[20] == -1           # mono-mono on the epipole: rejected
    assert k1["u_right"][21] >= 0 and m12[21] == 20                             # its stereo twin is not
    a, b, c, den = W.epipolar_line(k1["un_xy"][22], F12)
    assert a == 0 and b == 0 and den == 0 and (k1["desc"][22] == k2["desc"][22]).all() and m12[22] == -1


def test_transform_of_the_tiny_tree_meets_the_hand_written_expectations():
    import bow_ref as W
    import bow_scene as B
    tree = B.tiny_tree()
    feats = np.stack([B.bits(f) for f in B.TINY_EXPECT])
    for col, levelsup in ((1, 0), (2, 1), (3, 2), (4, 3), (4, 4), (4, 7)):       # levelsup >= levels: the root, 0
        node, word = W.transform(tree, feats, levelsup)
        assert word.tolist() == [e[0] for e in B.TINY_EXPECT.values()], levelsup
        assert node.tolist() == [e[col] for e in B.TINY_EXPECT.values()], levelsup
    assert W.transform_one(tree, B.bits(230), 1)[3] == 7 and (tree["desc"][7] == tree["desc"][8]).all()      # the tie: identical children, the first wins
    assert W.transform_one(tree, B.bits(21), 1)[1] == 0.0                       # the stopped word
    assert W.transform_one(tree, B.bits(130), 1)[2] is None                     # the shallow leaf: nid not set by the reference


def test_stream_vocabulary_gives_about_a_hundred_nodes(stream):
    import bow_scene as B
    node = B.stream_nodes(stream, 5)
    assert 70 <= len(set(node[node >= 0].tolist())) <= 100 and 10 < (node < 0).sum() < 150      # found: 87 nodes, 43 of 1505 keypoints stopped


def test_public_header_declares_the_new_calls_as_c(tmp_path):
    src = tmp_path / "surface.c"
    src.write_text('#include "sind_hip.h"\n'
                   "int (*const voc_create)(const sind_voc_tree*, int, int, int, sind_voc**) = &sind_voc_create;\n"
                   "int (*const voc_destroy)(sind_voc*) = &sind_voc_destroy;\n"
                   "int (*const voc_transform)(sind_voc*, const uint8_t* const*, const int*, int, int, int* const*, int* const*) = &sind_voc_transform;\n"
                   "int (*const by_bow)(sind_match*, const sind_match_bow*, int, float, int) = &sind_match_by_bow;\n"
                   "int (*const for_triangulation)(sind_match*, const sind_match_tri*, int, int, int) = &sind_match_for_triangulation;\n"
                   "int main(void) { return (int)(sizeof(sind_voc_tree) + sizeof(sind_match_bow) + sizeof(sind_match_tri)); }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_classes_have_the_new_methods():
    from sindslam_amd.matcher import ORBmatcher                                 # importing the modules loads no library
    from sindslam_amd.vocabulary import ORBVocabulary
    assert callable(ORBmatcher.SearchByBoW) and callable(ORBmatcher.SearchForTriangulation) and callable(ORBVocabulary.transform)
