"""GPU: sind_match_local_map (Frame::isInFrustum + MapPoint::PredictScale + ORBmatcher::SearchByProjection(F, vpMapPoints, th), reference
src/Frame.cc:340-396, src/MapPoint.cc:402-418, src/ORBmatcher.cc:45-137) and sind_match_by_projection_kf (src/ORBmatcher.cc:1472-1599) against
the Python restatement tests/localmap_ref.py.  All equalities; floats are compared as uint32 bit patterns.
The "plenty of matches" guards are half of what the restatement finds on these scenes (the found values stand beside them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NNRATIO = 0.8


def _matcher(cam, sc, B, cap=4096, cap_points=8192, checkOri=True):
    from sindslam_amd.matcher import ORBmatcher
    return ORBmatcher(cam[0], cam[1], cam[2], cam[3], cam[4], cam[6:10], sc, nnratio=NNRATIO, checkOri=checkOri, cap=cap, max_batch=B, cap_points=cap_points)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_frustum(got, fr):
    assert np.array_equal(got["in_view"], fr["in_view"])
    assert np.array_equal(got["level"], fr["level"])
    assert np.array_equal(_bits(got["proj_xyr"]), _bits(fr["proj_xyr"]))
    assert np.array_equal(_bits(got["view_cos"]), _bits(fr["view_cos"]))
    assert got["n_to_match"] == fr["n_to_match"]


@pytest.fixture(scope="module")
def stream_scenes(stream):
    import localmap_ref as R
    import localmap_scene as L
    out = []
    for t in (5, 6, 9):
        cam, sc, Tc, mp, cur = L.stream_local_map(stream, t, seed=t)
        out.append((cam, sc, Tc, mp, cur, R.frustum(cam, sc, Tc, mp)))
    return out


def test_frustum_outputs_on_the_branch_scene():
    import localmap_ref as R
    import localmap_scene as L
    cam, sc, Tc, mp, cur, expect = L.branch_scene()
    fr = R.frustum(cam, sc, Tc, mp)
    mt = _matcher(cam, sc, 1)
    got, = mt.SearchLocalPoints([(Tc, mp, cur)], 3.0)
    _assert_frustum(got, fr)
    assert fr["n_to_match"] == sum(e[0] == R.IN_VIEW for e in expect) > 90      # 12 classes of 8 in view: 96
    m, nm, _, _ = R.search_local(cam, sc, mp, cur, fr, 3.0, NNRATIO)
    assert got["nmatches"] == nm and np.array_equal(got["match_of_cur"], m) and nm > 12      # found: 25
    mt.close()


def test_frustum_outputs_on_the_stream_scene(stream_scenes):
    cam, sc = stream_scenes[0][0], stream_scenes[0][1]
    mt = _matcher(cam, sc, len(stream_scenes))
    got = mt.SearchLocalPoints([(Tc, mp, cur) for _, _, Tc, mp, cur, _ in stream_scenes], 3.0)
    for g, (_, _, _, mp, _, fr) in zip(got, stream_scenes):
        _assert_frustum(g, fr)
        assert fr["n_to_match"] > 2400                                           # found: 4913 / 4934 / 4852 of 5483 / 5464 / 5425 points
    mt.close()


def test_local_map_search_on_stream_frames_batched(stream_scenes):
    import localmap_ref as R
    cam, sc = stream_scenes[0][0], stream_scenes[0][1]
    mt = _matcher(cam, sc, len(stream_scenes))
    plenty = {1.0: 418, 3.0: 589, 5.0: 681}                                      # found: th 1: 836 / 889 / 953, th 3: 1178 / 1261 / 1332, th 5: 1363 / 1415 / 1455
    for th in (1.0, 3.0, 5.0):                                                   # the tracker's three values (Tracking.cc:1222-1227)
        got = mt.SearchLocalPoints([(Tc, mp, cur) for _, _, Tc, mp, cur, _ in stream_scenes], th)
        for g, (c, s, Tc, mp, cur, fr) in zip(got, stream_scenes):
            m, nm, _, _ = R.search_local(c, s, mp, cur, fr, th, NNRATIO)
            assert g["nmatches"] == nm and np.array_equal(g["match_of_cur"], m)
            assert nm > plenty[th]
        # found: 1017+ points per frame whose choice depends on earlier points, at every th.  Round 1 searches against the frame as it was on
        # entry, so one differing choice means a changing round 2 and a confirming round 3 (any match at all already gives 2)
        assert mt.last_rounds() >= 3
    mt.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_local_map_search_contended_keypoints_equal_distances_and_taken_flags(seed):
    import localmap_ref as R
    import localmap_scene as L
    cam, sc, Tc, mp, cur = L.stress_local_map(seed)
    fr = R.frustum(cam, sc, Tc, mp)
    mt = _matcher(cam, sc, 1)
    plenty = {1.0: 30, 3.0: 252, 5.0: 486}                                       # found: th 1: 75 / 60 / 71, th 3: 509 / 545 / 504, th 5: 1004 / 979 / 972
    for th in (1.0, 3.0, 5.0):
        got, = mt.SearchLocalPoints([(Tc, mp, cur)], th)
        _assert_frustum(got, fr)
        m, nm, choice, stats = R.search_local(cam, sc, mp, cur, fr, th, NNRATIO)
        assert got["nmatches"] == nm and np.array_equal(got["match_of_cur"], m)
        assert nm > plenty[th]
        if th >= 3.0:
            # the sequential dependence is really exercised: choices that differ from the choices against the frame as it was on entry
            # (found: th 3: 60 / 66 / 62, th 5: 228 / 224 / 234), and the same-level ratio rule fires both ways (th 5: 525 pairs, 57 rejected)
            _, _, choice0, _ = R.search_local(cam, sc, mp, cur, fr, th, NNRATIO, sequential=False)
            assert (choice != choice0).sum() > 0, "the scene is wrong, not the kernel"
            assert stats["rejected"] > 0 and stats["same_level"] > stats["rejected"]
            assert mt.last_rounds() >= 3                                         # round 1 = choice0, a differing choice changes round 2, round 3 confirms
    mt.close()


def test_ragged_batch_with_empty_frames_and_a_full_one():
    import localmap_ref as R
    import localmap_scene as L
    cam, sc, Tc, mp, cur = L.stress_local_map(4)
    n = len(mp["flags"])
    none = {k: v[:0] for k, v in mp.items()}
    blind = {k: (v[:0] if k != "grid_start" else np.zeros(3073, np.int32)) for k, v in cur.items()}
    few = {k: v[:500] for k, v in mp.items()}
    frames = [(Tc, none, cur), (Tc, mp, blind), (Tc, mp, cur), (Tc, few, cur)]
    mt = _matcher(cam, sc, 4, cap_points=n)                                      # frame 2 fills the reserved capacity exactly
    got = mt.SearchLocalPoints(frames, 5.0)
    for g, (T, p, c) in zip(got, frames):
        fr = R.frustum(cam, sc, T, p)
        _assert_frustum(g, fr)
        m, nm, _, _ = R.search_local(cam, sc, p, c, fr, 5.0, NNRATIO)
        assert g["nmatches"] == nm and np.array_equal(g["match_of_cur"], m)
    assert got[0]["nmatches"] == 0 and got[0]["n_to_match"] == 0 and (got[0]["match_of_cur"] == -1).all()
    assert got[1]["nmatches"] == 0 and got[1]["n_to_match"] > 1000 and len(got[1]["match_of_cur"]) == 0
    assert got[2]["nmatches"] > 475 and got[3]["nmatches"] > 94                  # found: 951 and 189; 2342 of 3000 points in view
    mt.close()


@pytest.mark.parametrize("th,orb_dist", [(10.0, 100), (3.0, 64)])                # the two calls of Tracking::Relocalization
@pytest.mark.parametrize("ori", [True, False])
def test_relocalisation_search_on_stream_pairs(stream, th, orb_dist, ori):
    import localmap_ref as R
    import localmap_scene as L
    scenes = [L.reloc_pair(stream, t, seed=t) for t in (4, 9)]                   # 15 % of the slots already found, 5 % of the keypoints held
    cam, sc = scenes[0][0], scenes[0][1]
    plenty = {(10.0, True): 336, (10.0, False): 383, (3.0, True): 197, (3.0, False): 201}   # found: 673 / 753, 766 / 836, 395 / 511, 403 / 528
    mt = _matcher(cam, sc, len(scenes), checkOri=ori)
    got = mt.SearchByProjectionKF([(Tc, kf, cur) for _, _, Tc, kf, cur in scenes], th, orb_dist)
    for (m, n), (c, s, Tc, kf, cur) in zip(got, scenes):
        assert (kf["valid"] == 0).sum() > 100 and cur["taken"].sum() > 30
        mo, no = R.search_kf(c, s, Tc, kf, cur, th, orb_dist, ori)
        assert n == no and np.array_equal(m, mo)
        assert n > plenty[(th, ori)]
        assert (m[cur["taken"] > 0] == -1).all()
    mt.close()


def test_argument_errors_launch_nothing():
    import localmap_ref as R
    import localmap_scene as L
    from sindslam_amd import SindError
    cam, sc, Tc, mp, cur = L.stress_local_map(5)
    small = {k: v[:60] for k, v in mp.items()}
    mt = _matcher(cam, sc, 1, cap_points=0)
    with pytest.raises(SindError, match="reserve"):
        mt.SearchLocalPoints([(Tc, small, cur)], 3.0)                            # before sind_match_reserve_map_points
    mt.reserve_map_points(64)
    with pytest.raises(SindError, match="capacity"):
        mt.SearchLocalPoints([(Tc, {k: v[:100] for k, v in mp.items()}, cur)], 3.0)   # 100 points > 64 reserved
    bad = dict(cur); bad["grid_idx"] = cur["grid_idx"].copy(); bad["grid_idx"][0] = len(cur["octave"])
    with pytest.raises(SindError, match="grid index"):
        mt.SearchLocalPoints([(Tc, small, bad)], 3.0)
    null = dict(small); null["desc"] = small["desc"][:0]
    with pytest.raises(SindError, match="null array"):
        mt.SearchLocalPoints([(Tc, null, cur)], 3.0)                             # NULL descriptors with 60 points
    kf = dict(x3Dw=mp["x3Dw"], max_dist=mp["max_dist"], min_dist=mp["min_dist"], valid=mp["flags"] & 1, angle=np.zeros(len(mp["flags"]), np.float32), desc=mp["desc"])
    cur_kf = dict(cur); cur_kf["angle"] = np.zeros(len(cur["octave"]), np.float32)
    with pytest.raises(SindError, match="grid index"):
        mt.SearchByProjectionKF([(Tc, kf, dict(cur_kf, grid_idx=bad["grid_idx"]))], 10.0, 100)
    with pytest.raises(SindError, match="capacity"):
        mt.SearchByProjectionKF([(Tc, {k: np.concatenate([v, v]) for k, v in kf.items()}, cur_kf)], 10.0, 100)   # 6000 slots > cap 4096
    got, = mt.SearchLocalPoints([(Tc, small, cur)], 3.0)                         # the handle still works
    fr = R.frustum(cam, sc, Tc, small)
    m, nm, _, _ = R.search_local(cam, sc, small, cur, fr, 3.0, NNRATIO)
    _assert_frustum(got, fr)
    assert got["nmatches"] == nm and np.array_equal(got["match_of_cur"], m)
    mt.close()
