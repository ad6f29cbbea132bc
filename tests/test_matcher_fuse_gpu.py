"""GPU: sind_match_fuse (both overloads of ORBmatcher::Fuse up to the graph tail, reference src/ORBmatcher.cc:825-949, :977-1079), sind_match_by_projection_sim3
(:290-403) and sind_match_by_sim3 (:1102-1326) against the Python restatement tests/fuse_ref.py.  All equalities on integer arrays.
The "plenty of matches" guards are half of what the restatement finds on these scenes (the found values stand beside them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S_FUSE, S_PROJ = 0.93, 1.08                                                  # scales of the similarities handed to FuseSim3 and SearchByProjectionSim3


def _matcher(cam, sc, B, cap=4096, cap_points=8192):
    from sindslam_amd.matcher import ORBmatcher
    return ORBmatcher(cam[0], cam[1], cam[2], cam[3], cam[4], cam[6:10], sc, cap=cap, max_batch=B, cap_points=cap_points)


def _assert_fuse(got, want):
    assert np.array_equal(got["best_idx"], want["best_idx"]) and np.array_equal(got["best_dist"], want["best_dist"]) and got["nfused"] == want["nfused"]


def _assert_all(mt, cam, sc, items, th_proj=10):
    """Fuse th 3, FuseSim3 th 4 and SearchByProjectionSim3 th 10 on one batch of (Tcw, mp, kf) against the restatement -> (nfused, nfused sim3, nmatches) per item"""
    import fuse_ref as F
    import fuse_scene as FS
    found = []
    got = mt.Fuse(items, 3.0)
    got3 = mt.FuseSim3([(FS.similarity(T, S_FUSE), mp, kf) for T, mp, kf in items], 4.0)
    gotp = mt.SearchByProjectionSim3([(FS.similarity(T, S_PROJ), mp, kf) for T, mp, kf in items], th_proj)
    for g, g3, (m, nm), (T, mp, kf) in zip(got, got3, gotp, items):
        w = F.fuse_search(cam, sc, T, mp, kf, 3.0, 0); _assert_fuse(g, w)
        w3 = F.fuse_search(cam, sc, FS.similarity(T, S_FUSE), mp, kf, 4.0, 1); _assert_fuse(g3, w3)
        mo, no, _, _ = F.search_kf_sim3(cam, sc, FS.similarity(T, S_PROJ), mp, kf, th_proj)
        assert nm == no and np.array_equal(m, mo)
        found.append((w["nfused"], w3["nfused"], no))
    return found


def _assert_sim3(mt, cam, sc, pairs, th=7.5):
    import fuse_ref as F
    found = []
    for (m12, nf), p in zip(mt.SearchBySim3(pairs, th), pairs):
        w12, wf = F.search_by_sim3(cam, sc, *p, th)[:2]
        assert nf == wf and np.array_equal(m12, w12)
        found.append(wf)
    return found


@pytest.fixture(scope="module")
def stream_scenes(stream):
    import fuse_scene as FS
    return [FS.stream_key_frame(stream, t, seed=t - 1) for t in (6, 7, 10)]


def test_branch_scene_all_calls_both_modes(stream):
    import fuse_ref as F
    import fuse_scene as FS
    cam, sc, Tc, mp, kf, expect = FS.branch_scene()
    mt = _matcher(cam, sc, 1)
    (nf, nf3, nm), = _assert_all(mt, cam, sc, [(Tc, mp, kf)])                 # the exits themselves: test_matcher_fuse_cpu.py
    assert nf > 1 and nf3 > 3 and nm > 15                                     # found: 3, 7 and 31 (112 of the 176 points are in view)
    *pair, n = FS.branch_sim3_pair(stream)
    why1 = F.search_by_sim3(*pair, 7.5)[4][:n]
    assert set(why1.tolist()) == {F.IN_VIEW, F.BEHIND, F.OUT_X, F.OUT_Y, F.OUT_DIST, F.NOT_CANDIDATE}
    nfound, = _assert_sim3(mt, pair[0], pair[1], [tuple(pair[2:])])
    assert nfound > 192                                                       # found: 384; of the 176 branch slots 104 in view, 8 / 16 / 16 / 24 / 8 by the exits
    mt.close()


def test_stream_scenes_batched(stream_scenes):
    cam, sc = stream_scenes[0][0], stream_scenes[0][1]
    mt = _matcher(cam, sc, len(stream_scenes))
    found = _assert_all(mt, cam, sc, [(Tc, mp, kf) for _, _, Tc, mp, kf in stream_scenes])
    # SearchByProjectionSim3 ran last: hundreds of points per item whose choice depends on earlier points (test_matcher_fuse_cpu.py), so round 1 = the choices against
    # vpMatched on entry, a differing choice changes round 2, round 3 confirms
    assert mt.last_rounds() >= 3
    for nf, nf3, nm in found:
        assert nf > 724 and nf3 > 761 and nm > 372                             # found: 1449 / 1520 / 1706, 1523 / 1605 / 1832, 745 / 805 / 908
    mt.close()


def test_search_by_sim3_on_stream_pairs_batched(stream):
    import fuse_scene as FS
    scenes = [FS.sim3_pair(stream, 6, seed=6, scale=1.08), FS.sim3_pair(stream, 6, seed=7, scale=0.93), FS.sim3_pair(stream, 7, seed=8, scale=1.08)]
    cam, sc = scenes[0][0], scenes[0][1]
    assert len({len(s[7]["valid"]) for s in scenes} | {len(s[8]["valid"]) for s in scenes}) > 1          # sides of unequal size
    mt = _matcher(cam, sc, len(scenes), cap_points=0)                                                    # needs no map-point reservation
    found = _assert_sim3(mt, cam, sc, [s[2:] for s in scenes])
    assert min(found) > 210                                                   # found: 420 / 456 / 471
    mt.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuse_and_projection_contended_keypoints_and_equal_distances(seed):
    import fuse_ref as F
    import fuse_scene as FS
    cam, sc, Tc, mp, kf = FS.stress_key_frame(seed)
    mt = _matcher(cam, sc, 1)
    (nf, nf3, nm), = _assert_all(mt, cam, sc, [(Tc, mp, kf)])
    assert nf > 23 and nf3 > 110 and nm > 383                                 # found: 57 / 47 / 46, 228 / 221 / 224, 794 / 766 / 777
    assert mt.last_rounds() >= 3
    # equal distances: matched points with a second candidate at the best distance later in the walk; strict < kept the first
    w3 = F.fuse_search(cam, sc, FS.similarity(Tc, S_FUSE), mp, kf, 4.0, 1)
    T, Ow = F._pose(FS.similarity(Tc, S_FUSE), 1); ties = 0
    for i in np.nonzero(w3["best_idx"] >= 0)[0]:
        _, u, v, _, lv = F.project(F.FUSE_SIM3, cam, sc, T, Ow, mp["x3Dw"][i], mp["normal"][i], mp["max_dist"][i], mp["min_dist"][i])
        cand = [k for k in F.kf_features_in_area(cam, kf, u, v, np.float32(np.float32(4.0) * sc[lv])) if lv - 1 <= kf["octave"][k] <= lv]
        same = [k for k in cand if F.hamming(mp["desc"][i], kf["desc"][k]) == w3["best_dist"][i]]
        assert same[0] == w3["best_idx"][i]
        ties += len(same) > 1
    assert ties > 3                                                           # found: 7 / 7 / 7
    mt.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_search_by_sim3_contended_keypoints_and_equal_distances(stream, seed):
    import fuse_ref as F
    import fuse_scene as FS
    cam, sc, *pair = FS.stress_sim3_pair(stream, seed)
    mt = _matcher(cam, sc, 1, cap_points=0)
    nfound, = _assert_sim3(mt, cam, sc, [tuple(pair)])
    vn1, vn2 = F.search_by_sim3(cam, sc, *pair, 7.5)[2:4]
    assert nfound > 87 and (vn1 >= 0).sum() - nfound > 76                     # found: 195 / 185 / 174 agreeing, 163 / 162 / 153 one-way only
    mt.close()


def test_ragged_batch_empty_items_a_full_one_and_block_edges():
    import fuse_scene as FS
    cam, sc, Tc, mp, kf = FS.stress_key_frame(4)
    n = len(mp["valid"])
    none = {k: v[:0] for k, v in mp.items()}
    blind = {k: (v[:0] if k != "grid_start" else np.zeros(3073, np.int32)) for k, v in kf.items()}
    cut = lambda c: {k: v[:c] for k, v in mp.items()}
    items = [(Tc, none, kf), (Tc, mp, blind), (Tc, mp, kf), (Tc, cut(65), kf), (Tc, cut(257), kf)]      # 65, 257: one past a block of k_search_kf, of k_project_kf
    mt = _matcher(cam, sc, len(items), cap_points=n)                                                     # item 2 fills the reserved capacity exactly
    found = _assert_all(mt, cam, sc, items)
    assert found[0] == (0, 0, 0) and found[1] == (0, 0, 0)
    assert found[2][0] > 26 and found[2][1] > 110 and found[2][2] > 370 and found[4][1] > 7      # found: 52, 221, 740; 14 of the 257 points
    mt.close()


def test_fractional_frame_bounds_are_truncated_for_the_key_frame():
    """a distorted camera: the frame's bounds are not integers, the key frame keeps them as int, and the grid cell size stays the frame's"""
    import fuse_scene as FS
    cam, sc, Tc, mp, kf = FS.stress_key_frame(6)
    cam = cam.copy(); cam[6:10] = (-12.7, 655.4, -9.2, 489.9)
    mt = _matcher(cam, sc, 1)
    (nf, nf3, nm), = _assert_all(mt, cam, sc, [(Tc, mp, kf)])
    assert nf > 25 and nf3 > 106 and nm > 359                                 # found: 50, 212, 719 (721 with the cell size of the truncated bounds)
    mt.close()


def test_search_by_sim3_unequal_and_empty_sides(stream):
    import fuse_scene as FS
    cam, sc, T1, T2, s12, R12, t12, s1, s2 = FS.sim3_pair(stream, 6, seed=6)
    empty = {k: (v[:0] if k != "grid_start" else np.zeros(3073, np.int32)) for k, v in s1.items()}
    assert len(s1["valid"]) != len(s2["valid"])
    mt = _matcher(cam, sc, 3, cap_points=0)
    found = _assert_sim3(mt, cam, sc, [(T1, T2, s12, R12, t12, s1, s2), (T1, T2, s12, R12, t12, empty, s2), (T1, T2, s12, R12, t12, s1, empty)])
    assert found[0] > 210 and found[1:] == [0, 0]                             # found: 420
    mt.close()


def test_argument_errors_launch_nothing(stream):
    import fuse_ref as F
    import fuse_scene as FS
    from sindslam_amd import SindError
    cam, sc, Tc, mp, kf = FS.stress_key_frame(5)
    small = {k: v[:60] for k, v in mp.items()}
    Scw = FS.similarity(Tc, S_PROJ)
    mt = _matcher(cam, sc, 2, cap_points=0)
    calls = [lambda it: mt.Fuse(it, 3.0), lambda it: mt.FuseSim3(it, 4.0), lambda it: mt.SearchByProjectionSim3(it, 10)]
    for call in calls:
        with pytest.raises(SindError, match="reserve"):
            call([(Tc, small, kf)])                                           # before sind_match_reserve_map_points
    mt.reserve_map_points(64)
    bad_grid = dict(kf, grid_idx=kf["grid_idx"].copy()); bad_grid["grid_idx"][0] = len(kf["octave"])
    bad_oct = dict(kf, octave=kf["octave"].copy()); bad_oct["octave"][7] = len(sc)
    null = dict(small, desc=small["desc"][:0])
    for call in calls:
        for item, what in ((({k: v[:100] for k, v in mp.items()}, kf), "capacity"), ((small, bad_grid), "grid index"), ((null, kf), "null array"), ((small, bad_oct), "octave")):
            with pytest.raises(SindError, match=what):
                call([(Tc, small, kf), (Tc, *item)])                          # the second item is the bad one: the first is not run either
    # the outputs stay as the caller left them
    import ctypes as C
    from sindslam_amd import matcher as M
    from sindslam_amd._lib import lib
    a = M._points_kf(small, bad_grid, u_right=True)
    a.update(Tcw=np.ascontiguousarray(Tc, np.float32), best_idx=np.full(60, 77, np.int32), best_dist=np.full(60, 77, np.int32), nfused=np.full(1, 77, np.int32))
    with pytest.raises(SindError, match="grid index"):
        mt._call("sind_match_fuse", M._Fuse, [a], C.c_float(3.0), 0)
    assert (a["best_idx"] == 77).all() and (a["best_dist"] == 77).all() and a["nfused"][0] == 77
    # SearchBySim3: over capacity, malformed grid, NULL descriptors, octave
    cam2, sc2, T1, T2, s12, R12, t12, s1, s2 = FS.sim3_pair(stream, 6, seed=6)
    ms = _matcher(cam2, sc2, 1, cap=len(s1["valid"]) - 1, cap_points=0)
    with pytest.raises(SindError, match="capacity"):
        ms.SearchBySim3([(T1, T2, s12, R12, t12, s1, s2)], 7.5)
    ms.close()
    ms = _matcher(cam2, sc2, 1, cap_points=0)
    g = s2["grid_idx"].copy(); g[0] = len(s2["valid"])
    o = s1["octave"].copy(); o[3] = -1
    for pair, what in (((s1, dict(s2, grid_idx=g)), "grid index"), ((dict(s1, mp_desc=s1["mp_desc"][:0]), s2), "null array"), ((dict(s1, octave=o), s2), "octave")):
        with pytest.raises(SindError, match=what):
            ms.SearchBySim3([(T1, T2, s12, R12, t12, *pair)], 7.5)
    (m12, nf), = ms.SearchBySim3([(T1, T2, s12, R12, t12, s1, s2)], 7.5)      # the handles still work
    w12, wf = F.search_by_sim3(cam2, sc2, T1, T2, s12, R12, t12, s1, s2, 7.5)[:2]
    assert nf == wf and np.array_equal(m12, w12)
    ms.close()
    _assert_all(mt, cam, sc, [(Tc, small, kf)])
    mt.close()


def test_one_handle_serves_old_and_new_searches_in_turn(stream):
    import fuse_scene as FS
    import localmap_ref as R
    import localmap_scene as L
    cam, sc, Tc, mp, cur = L.stress_local_map(2)
    fr = R.frustum(cam, sc, Tc, mp)
    m, nm, _, _ = R.search_local(cam, sc, mp, cur, fr, 3.0, 0.8)
    _, _, _, pts, kf = FS.stress_key_frame(3)
    pair = FS.stress_sim3_pair(stream, 1)[2:]
    from sindslam_amd.matcher import ORBmatcher
    mt = ORBmatcher(cam[0], cam[1], cam[2], cam[3], cam[4], cam[6:10], sc, nnratio=0.8, cap=4096, max_batch=1, cap_points=8192)
    for _ in range(2):                                                        # old, new, and back
        got, = mt.SearchLocalPoints([(Tc, mp, cur)], 3.0)
        assert got["nmatches"] == nm and np.array_equal(got["match_of_cur"], m)
        _assert_all(mt, cam, sc, [(Tc, pts, kf)])
        _assert_sim3(mt, cam, sc, [pair])
    mt.close()
