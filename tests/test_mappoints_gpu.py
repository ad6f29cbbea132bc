"""GPU: sind_match_triangulate and sind_match_update_points (csrc/match_mappoints.hip: k_tri_points, k_mp_descriptor, k_mp_normal) against the host library's
sindh_triangulate and sindh_update_points (the same source csrc/host/map_points.hpp; the descriptor choice transcribed literally there, found by bisection here) as bit
patterns on every output; the literal cases of the CPU test; independence of the items of a batch and of the workspace's growth; the error paths and the limits; the
calls on a handle shared with other matcher calls; and the local mapper's step on a toy map through sindslam_amd.mapping and sindslam_amd.optimizer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
CAP = 512
MPU_MAX_KF, MPU_MAX_MP, MPU_MAX_OBS = 4096, 65536, 1 << 20             # limits of csrc/host/map_points.hpp


@pytest.fixture(scope="module")
def matcher4():
    import mappoints_scene as SC
    from sindslam_amd.matcher import ORBmatcher
    K = SC.K5
    mt = ORBmatcher(float(K[0]), float(K[1]), float(K[2]), float(K[3]), float(K[4]), (0, 640, 0, 480), SC.SCALE, nnratio=0.6, checkOri=True, cap=CAP, max_batch=4, cap_points=CAP)
    yield mt
    mt.close()


def _same_tri(mt, pairs, what):
    import mappoints_scene as SC
    got = mt.Triangulate(pairs); ref = SC.HostMap().Triangulate(pairs)
    for k, (g, r) in enumerate(zip(got, ref)):
        SC.assert_same(g, r, SC.TRI_OUT, (what, k))
    return got


def _same_mp(mt, items, what):
    import mappoints_scene as SC
    got = mt.UpdateMapPoints(items); ref = SC.HostMap().UpdateMapPoints(items)
    for k, (g, r) in enumerate(zip(got, ref)):
        SC.assert_same(g, r, SC.MP_OUT, (what, k))
    return got


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_triangulate_equals_the_host_library_bit_for_bit(matcher4, kind):
    """one lane per match, 64 lanes per block: 0, 1, 63, 64, 65 and 257 matches per pair cross wave and block edges; B = 4 with unequal pairs puts the seam between two
    pairs inside a wave (63 | 1 | 65 | 0 | 40: the second pair is one lane)"""
    import mappoints_scene as SC
    seed = {"mono": 100, "stereo": 200, "mixed": 300}[kind]
    exact = dict(unmatched=0, wrong=0.08)
    for k, n in enumerate((0, 1, 63, 64, 65, 257)):
        p = SC.tri_scene(seed + k, n, kind, **exact)
        g = _same_tri(matcher4, [p], (kind, n))[0]
        assert (g["status"] >= 0).sum() == n
    batch = [SC.tri_scene(seed + 10, 63, kind, **exact), SC.tri_scene(seed + 11, 1, kind, baseline=0.02, **exact), SC.tri_scene(seed + 12, 65, kind, baseline=0.02, **exact), SC.tri_scene(seed + 13, 0, kind)]
    got = _same_tri(matcher4, batch, (kind, "batch"))
    _same_tri(matcher4, [batch[3], SC.tri_scene(seed + 14, 40, kind), batch[1]], (kind, "an empty pair first"))
    seen = {h for g in got for h in g["how"].tolist()}
    assert 0 in seen and (kind == "mono" or 1 in seen or 2 in seen)
    assert matcher4.Triangulate([]) == []


def test_triangulate_literal_cases_equal_the_host_library(matcher4):
    import mappoints_scene as SC
    cases = SC.tri_literal_cases(); names = list(cases)
    for a in range(0, len(names), 4):
        got = _same_tri(matcher4, [cases[n][0] for n in names[a:a + 4]], names[a:a + 4])
        for n, g in zip(names[a:a + 4], got):
            assert (int(g["status"][0]), int(g["how"][0])) == cases[n][1:], n


@pytest.mark.parametrize("flags", [(True, True), (True, False), (False, True)])
def test_update_points_equals_the_host_library_bit_for_bit(matcher4, flags):
    """one wave per point, four points per block: 1, 255, 256 and 257 points per item; lists of 1, 2, 3, 63, 64 (lanes in registers), 65 and 130 observations (chunks of 64,
    a partial last chunk); one item mixing all of them; each flag alone and both"""
    import mappoints_scene as SC
    counts = [1, 2, 3, 63, 64, 65, 130]
    for k, c in enumerate(counts):
        _same_mp(matcher4, [SC.mp_scene(400 + k, [c] * 5, flags=flags)], ("observations", c))
    rng = np.random.RandomState(7)
    for k, n in enumerate((1, 255, 256, 257)):
        _same_mp(matcher4, [SC.mp_scene(420 + k, rng.randint(0, 9, n).tolist(), flags=flags)], ("points", n))
    mix = SC.mp_scene(430, counts + [0] + counts[::-1], bad=0.3, flags=flags)
    g = _same_mp(matcher4, [mix, SC.mp_scene(431, [4] * 9, flags=flags), SC.mp_scene(432, [], flags=flags)], "mixed")[0]
    if not flags[0]:
        assert (g["desc"] == 0xAB).all() and (g["best_obs"] == -1).all()
    if not flags[1]:
        assert (g["normal"] == 7.0).all() and (g["updated"] == 0).all()
    assert matcher4.UpdateMapPoints([]) == []


def test_update_points_literal_cases_equal_the_host_library(matcher4):
    import mappoints_scene as SC
    cases = SC.mp_literal_cases(); names = list(cases)
    for a in range(0, len(names), 4):
        got = _same_mp(matcher4, [cases[n][0] for n in names[a:a + 4]], names[a:a + 4])
        for n, g in zip(names[a:a + 4], got):
            assert g["best_obs"].tolist() == cases[n][1], n
    g = matcher4.UpdateMapPoints([cases["all_bad"][0]])[0]
    assert (g["desc"] == 0xAB).all() and g["updated"][0] == 1             # every observer bad: mDescriptor stays, the normal is still formed


def test_items_of_a_batch_are_independent_and_the_workspace_may_grow(matcher4):
    """the same item alone, first and last gives the same bytes; a small call, a large one (the workspace grows), the small one again"""
    import mappoints_scene as SC
    a = SC.mp_scene(501, [3, 70, 1, 0, 8]); b = SC.mp_scene(502, [5] * 40, bad=0.3); c = SC.mp_scene(503, [2, 66])
    alone = matcher4.UpdateMapPoints([a])[0]
    for items, k in (([a, b, c], 0), ([b, a], 1), ([c, b, a], 2), ([a, a], 1)):
        SC.assert_same(matcher4.UpdateMapPoints(items)[k], alone, SC.MP_OUT, ("neighbours", len(items), k))
    _same_mp(matcher4, [SC.mp_scene(504, [6] * 3000), b], "grown")       # 18 000 observations: beyond the first allocation
    SC.assert_same(matcher4.UpdateMapPoints([a])[0], alone, SC.MP_OUT, "after the growth")
    p = SC.tri_scene(511, 30); q = SC.tri_scene(512, 70, "stereo"); r = SC.tri_scene(513, 5, "mono")
    alone = matcher4.Triangulate([p])[0]
    for pairs, k in (([p, q, r], 0), ([q, p], 1), ([r, q, p], 2)):
        SC.assert_same(matcher4.Triangulate(pairs)[k], alone, SC.TRI_OUT, ("pairs", len(pairs), k))
    big = [SC.tri_scene(514 + k, 500, unmatched=0) for k in range(3)]     # 1 500 matches: beyond the first allocation
    _same_tri(matcher4, big, "grown")
    SC.assert_same(matcher4.Triangulate([p])[0], alone, SC.TRI_OUT, "after the growth")


def test_error_paths_launch_nothing_and_leave_the_outputs_untouched(matcher4):
    import mappoints_scene as SC
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import mappoints_items, triangulate_items
    good = SC.mp_scene(601, [2, 3, 1])

    def refused_mp(items, rc, what):
        arr, keep = mappoints_items(items)
        assert lib().sind_match_update_points(matcher4._h, arr, len(items)) == rc, what
        for a in keep:
            assert (a["desc_out"] == 0xAB).all() and (a["best_obs"] == -1).all() and (a["normal_out"] == 7.0).all() and (a["max_dist"] == 7.0).all() and (a["min_dist"] == 7.0).all() and \
                (a["updated"] == 0).all(), what

    for name, bad in SC.mp_bad_items().items():
        refused_mp([good, bad], SIND_E_ARG, name)
    refused_mp([good] * 5, SIND_E_CAPACITY, "max_batch is 4")
    refused_mp([good, SC.mp_scene(602, [1, 2], n_kf=MPU_MAX_KF + 1)], SIND_E_CAPACITY, "key frames")
    many = SC.mp_item([dict(x3Dw=[0, 0, 5.0], obs=[], ref=-1)] * (MPU_MAX_MP + 1), 4)
    refused_mp([good, many], SIND_E_CAPACITY, "points")
    n = MPU_MAX_OBS + 1                                                 # one point with 2^20 + 1 observations (of 4 097 key frames in turn: the limits are decided before the contents)
    wide = dict(Ow=np.zeros((4, 3), np.float32), x3Dw=np.array([[0, 0, 5.0]], np.float32), obs_start=np.array([0, n], np.int32), obs_kf=np.zeros(n, np.int32), obs_bad=np.zeros(n, np.uint8),
                obs_octave=np.zeros(n, np.int32), obs_desc=np.zeros((n, 32), np.uint8), ref_obs=np.zeros(1, np.int32), desc=np.full((1, 32), 0xAB, np.uint8), normal=np.full((1, 3), 7.0, np.float32),
                max_dist=np.full(1, 7.0, np.float32), min_dist=np.full(1, 7.0, np.float32))
    refused_mp([good, wide], SIND_E_CAPACITY, "observations")
    arr, keep = mappoints_items([good])
    assert lib().sind_match_update_points(matcher4._h, None, 1) == SIND_E_ARG and lib().sind_match_update_points(matcher4._h, arr, -1) == SIND_E_ARG
    _same_mp(matcher4, [good], "after the errors")

    ok = SC.tri_scene(611, 9)

    def refused_tri(pairs, rc, what):
        arr, keep = triangulate_items(pairs)
        for a in keep:
            a["x3D"][:] = 7.0; a["how"][:] = 77; a["status"][:] = 77; a["nnew"][:] = 77
        assert lib().sind_match_triangulate(matcher4._h, arr, len(pairs)) == rc, what
        for a in keep:
            assert (a["x3D"] == 7.0).all() and (a["how"] == 77).all() and (a["status"] == 77).all() and a["nnew"][0] == 77, what

    for name, bad in SC.tri_bad_pairs().items():
        refused_tri([ok, bad], SIND_E_ARG, name)
    refused_tri([ok] * 5, SIND_E_CAPACITY, "max_batch is 4")
    refused_tri([ok, SC.tri_scene(612, CAP + 1, unmatched=0.9)], SIND_E_CAPACITY, "cap_last")
    refused_tri([ok, SC.tri_scene(613, CAP - 2, unmatched=0.9, extra=5)], SIND_E_CAPACITY, "cap_cur")
    arr, keep = triangulate_items([ok])
    assert lib().sind_match_triangulate(matcher4._h, None, 1) == SIND_E_ARG and lib().sind_match_triangulate(matcher4._h, arr, -1) == SIND_E_ARG
    _same_tri(matcher4, [ok], "after the errors")


def test_calls_on_a_handle_shared_with_other_matcher_calls(matcher4):
    """one PoseOptimization before and one after, with unchanged results"""
    import mappoints_scene as SC
    import poseopt_scene as P
    s = P.scene(5, 60)
    before = matcher4.PoseOptimization([s])[0]
    p = SC.tri_scene(701, 90); it = SC.mp_scene(702, [4, 66, 9] * 10)
    _same_tri(matcher4, [p], "shared"); _same_mp(matcher4, [it], "shared")
    after = matcher4.PoseOptimization([s])[0]
    for k in ("Tcw", "outlier", "round_chi2", "round_lambda", "round_pose"):
        assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k
    _same_tri(matcher4, [p], "shared, again"); _same_mp(matcher4, [it], "shared, again")


def test_local_mapping_step_on_a_toy_map(matcher4):
    """create_new_map_points, Fuse with update_after_fuse, LocalBundleAdjustment with apply_local_ba and update_after_local_ba, once with every call on the device handle and
    once with Triangulate, UpdateMapPoints and LocalBundleAdjustment on their host twins (the two searches have no twin in the host library and stay on the device in both
    runs): the maps are equal, and the updated points feed SearchLocalPoints"""
    import copy

    import localba_scene as LS
    import mappoints_scene as SC

    class Hybrid(SC.HostMap):
        max_batch = 4
        SearchForTriangulation = lambda self, pairs, bOnlyStereo=False: self._on_device("SearchForTriangulation", pairs, bOnlyStereo)
        Fuse = lambda self, items, th=3.0: matcher4.Fuse(items, th)
        LocalBundleAdjustment = lambda self, items: LS.HostBA().LocalBundleAdjustment(items)

        def _on_device(self, name, *args):
            keep, matcher4.checkOri = matcher4.checkOri, self.checkOri
            try:
                return getattr(matcher4, name)(*args)
            finally:
                matcher4.checkOri = keep

    kfs, mps, cur = SC.toy_map(5)
    Kd, Pd = copy.deepcopy(kfs), copy.deepcopy(mps); Kh, Ph = copy.deepcopy(kfs), copy.deepcopy(mps)
    new_d, fused_d, res_d = SC.local_mapping_step(matcher4, Kd, Pd, cur)
    new_h, fused_h, res_h = SC.local_mapping_step(Hybrid(), Kh, Ph, cur)
    assert new_d == new_h and len(new_d) >= 60 and fused_d == fused_h and fused_d >= 20 and res_d["erase"] == res_h["erase"]
    SC.same_maps((Kd, Pd), (Kh, Ph))
    assert matcher4.checkOri is True
    ids = [m for m in sorted(Pd) if not Pd[m].get("bad") and Pd[m].get("normal") is not None][:CAP]
    mp = dict(x3Dw=np.array([Pd[m]["x3Dw"] for m in ids], np.float32), normal=np.array([Pd[m]["normal"] for m in ids], np.float32), max_dist=np.array([Pd[m]["max_dist"] for m in ids], np.float32),
              min_dist=np.array([Pd[m]["min_dist"] for m in ids], np.float32), flags=np.ones(len(ids), np.uint8), desc=np.array([Pd[m]["desc"] for m in ids], np.uint8))
    kf = Kd[cur]; gs, gi = SC.build_grid(kf["un_xy"])
    r = matcher4.SearchLocalPoints([(kf["Tcw"], mp, dict(un_xy=kf["un_xy"], octave=kf["octave"], u_right=kf["u_right"], desc=kf["desc"], grid_start=gs, grid_idx=gi))], th=3)[0]
    seen = sum(1 for m in ids if cur in Pd[m]["obs"])
    print("SearchLocalPoints on the updated map:", r["nmatches"], "matches,", int(r["in_view"].sum()), "of", len(ids), "points in view,", seen, "observed by the key frame")
    assert r["nmatches"] >= 0.8 * seen and seen >= 100
    hit = [(int(i), int(j)) for i, j in enumerate(r["match_of_cur"]) if j >= 0]
    assert sum(1 for i, j in hit if Pd[ids[j]]["obs"].get(cur) == i) >= 0.9 * len(hit)      # the keypoint a point was matched to is the one that observes it
