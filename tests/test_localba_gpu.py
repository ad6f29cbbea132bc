"""GPU: sind_match_local_ba (Optimizer::LocalBundleAdjustment of every item in one launch, csrc/match_localba.hip) against the host library's sindh_local_ba (the same
source, csrc/host/local_ba.hpp, with the plain sequential executor) as bit patterns, every output and diagnostic; against the Python restatement
tests/localba_ref.py; the literal cases of the CPU test; independence of the items of a batch and of the workspace's growth; the error paths and the limits; the call
on a handle shared with other matcher calls; and the local mapper's step on a small synthetic map through sindslam_amd.optimizer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
THREADS = 512                                                           # LBA_THREADS of csrc/match.hpp: the lanes that stride over the elements of a phase
LBA_MAX_POSES, LBA_MAX_KF = 256, 4096                                   # limits of csrc/host/local_ba.hpp


def _matcher(B):
    import localba_scene as SC
    import sim3_scene as S3
    from sindslam_amd.matcher import ORBmatcher
    K = SC.K5
    return ORBmatcher(float(K[0]), float(K[1]), float(K[2]), float(K[3]), float(K[4]), (0, 640, 0, 480), S3.scale_factors(), nnratio=0.75, checkOri=True, cap=192, max_batch=B)


@pytest.fixture(scope="module")
def matcher4():
    mt = _matcher(4)
    yield mt
    mt.close()


def _same(mt, items, what):
    import localba_scene as SC
    got = mt.LocalBundleAdjustment(items); ref = SC.HostBA().LocalBundleAdjustment(items)
    for k, (g, r) in enumerate(zip(got, ref)):
        SC.assert_same(g, r, (what, k))
    return got


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_device_equals_the_host_library_bit_for_bit(matcher4, kind):
    """The kernel has no chunk and no second code path: a phase is `lanes stride over elements, one barrier`, so what can go wrong with size is the stride itself
    (elements below, at and above THREADS = 512 lanes) and the size of the reduced system.  Free poses P = 1, 2, 10, 11: 6 P = 6, 12, 60 (below 64), 66 (above 64; no P
    gives 64); points 63, 64, 65 and 513 (one past THREADS, with 2 052 edges: also more edges than four strides); edges per pose and in total follow from these:
    P = 1 with 511, 512, 513 points all seen by the one free pose puts that pose's edge list, the point count and the pair list one below, at and one above THREADS."""
    import localba_scene as SC
    seed = {"mono": 100, "stereo": 200, "mixed": 300}[kind]
    batches = [[SC.scene(seed + 1, 1, 2, 63, kind=kind, outliers=3), SC.scene(seed + 2, 2, 1, 64, kind=kind, outliers=3), SC.scene(seed + 3, 10, 2, 65, kind=kind, outliers=6, obs_per_point=5)],
               [SC.scene(seed + 4, 11, 1, 40, kind=kind, outliers=4, obs_per_point=6), SC.scene(seed + 5, 2, 2, THREADS + 1, kind=kind, outliers=20)],
               [SC.scene(seed + 6, 1, 2, THREADS - 1, kind=kind, outliers=9), SC.scene(seed + 7, 1, 2, THREADS, kind=kind, outliers=9), SC.scene(seed + 8, 1, 2, THREADS + 1, kind=kind, outliers=9)]]
    for b, items in enumerate(batches):
        got = _same(matcher4, items, (kind, b))
        assert all(g["n_stages"] == 2 and g["erase"].sum() >= s["planted"].sum() for g, s in zip(got, items))


def test_largest_scene_equals_the_host_library(matcher4):
    """about 1 100 points x 4 observations, 6 free poses and 2 fixed cameras"""
    import localba_scene as SC
    s = SC.scene(400, 6, 2, 1100, kind="mixed", outliers=40, obs_per_point=4)
    g = _same(matcher4, [s], "large")[0]
    assert g["n_stages"] == 2 and len(s["obs_kf"]) == 4400


def test_device_equals_the_restatement(matcher4):
    import localba_ref as R
    import localba_scene as SC
    s = SC.scene(2, 4, 1, 30, kind="mixed", outliers=4)
    SC.assert_same(matcher4.LocalBundleAdjustment([s])[0], R.local_ba(s, SC.K5), "restatement")


def test_literal_cases_equal_the_host_library(matcher4):
    import localba_scene as SC
    cases = SC.literal_cases()
    names = list(cases)
    for a in range(0, len(names), 4):
        _same(matcher4, [cases[n] for n in names[a:a + 4]], names[a:a + 4])
    g = matcher4.LocalBundleAdjustment([cases["depth0_stop"], cases["n_obs0"]])
    assert np.isfinite(g[0]["Tcw"]).all() and np.isfinite(g[0]["x3Dw"]).all() and g[0]["n_stages"] == 1 and g[1]["n_stages"] == 0
    assert matcher4.LocalBundleAdjustment([]) == []


def test_items_of_a_batch_are_independent_and_the_workspace_may_grow(matcher4):
    """the same item alone, first, last and between other neighbours gives the same bytes; a small call, a large one (the workspace grows), the small one again"""
    import localba_scene as SC
    a = SC.scene(501, 3, 1, 20, kind="mixed", outliers=2); b = SC.scene(502, 5, 2, 70, kind="stereo", outliers=5); c = SC.scene(503, 2, 1, 33, kind="mono", outliers=3)
    alone = matcher4.LocalBundleAdjustment([a])[0]
    for items, k in (([a, b, c], 0), ([b, a], 1), ([c, b, a, c], 2), ([a, a], 1)):
        SC.assert_same(matcher4.LocalBundleAdjustment(items)[k], alone, ("neighbours", len(items), k))
    big = SC.scene(504, 8, 2, 900, kind="mixed", outliers=30, obs_per_point=5)
    _same(matcher4, [big, b], "grown")
    SC.assert_same(matcher4.LocalBundleAdjustment([a])[0], alone, "after the growth")


def test_error_paths_launch_nothing_and_leave_the_outputs_untouched(matcher4):
    import localba_scene as SC
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import localba_items
    good = SC.scene(601, 3, 1, 8, kind="mixed")
    for name, bad in SC.bad_items().items():
        arr, keep = localba_items([good, bad])
        for a in keep:
            a["Tcw_out"][:] = 7.0; a["x3Dw_out"][:] = 7.0; a["erase"][:] = 7; a["n_stages"][:] = 7
        assert lib().sind_match_local_ba(matcher4._h, arr, 2) == SIND_E_ARG, name
        for a in keep:
            assert (a["Tcw_out"] == 7.0).all() and (a["x3Dw_out"] == 7.0).all() and (a["erase"] == 7).all() and a["n_stages"][0] == 7, name
    arr, keep = localba_items([good])
    assert lib().sind_match_local_ba(matcher4._h, None, 1) == SIND_E_ARG and lib().sind_match_local_ba(matcher4._h, arr, -1) == SIND_E_ARG
    arr, keep = localba_items([good] * 5)
    assert lib().sind_match_local_ba(matcher4._h, arr, 5) == SIND_E_CAPACITY                      # max_batch is 4
    for n_local, n_fixed in ((LBA_MAX_POSES + 1, 0), (2, LBA_MAX_KF - 1)):                        # one free pose, one key frame beyond the limit
        many = SC.scene(602, n_local, n_fixed, 2, kind="mono", obs_per_point=2)
        arr, keep = localba_items([good, many])
        keep[0]["Tcw_out"][:] = 7.0
        assert lib().sind_match_local_ba(matcher4._h, arr, 2) == SIND_E_CAPACITY
        assert (keep[0]["Tcw_out"] == 7.0).all()
    SC.assert_same(matcher4.LocalBundleAdjustment([good])[0], SC.HostBA().LocalBundleAdjustment([good])[0], "after the errors")


def test_call_on_a_handle_shared_with_other_matcher_calls(matcher4):
    """one PoseOptimization before and one after, with unchanged results"""
    import localba_scene as SC
    import poseopt_scene as P
    s = P.scene(5, 60)
    before = matcher4.PoseOptimization([s])[0]
    a = SC.scene(701, 4, 1, 40, kind="mixed", outliers=4)
    _same(matcher4, [a], "shared")
    after = matcher4.PoseOptimization([s])[0]
    for k in ("Tcw", "outlier", "round_chi2", "round_lambda", "round_pose"):
        assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k
    _same(matcher4, [a], "shared, again")


def test_local_mapping_step_on_a_small_map(matcher4):
    """6 key frames and 150 points, covisibility from the shared observations, poses and points perturbed, 5 % planted outlier observations: the erased pairs are the planted
    ones, and the mean reprojection error of the kept observations is the host twin's figure (device == host), which lies below the pixel noise's level"""
    import copy

    import localba_scene as SC
    from sindslam_amd import optimizer as O
    kfs, mps, planted = SC.toy_map(3, share=0.95)
    ref = O.LocalBundleAdjustment(SC.HostBA(), 5, kfs, mps)
    got = O.LocalBundleAdjustment(matcher4, 5, kfs, mps)
    assert got["erase"] == ref["erase"] and set(got["erase"]) == planted and len(planted) >= 25
    for k in ref["poses"]:
        assert got["poses"][k].tobytes() == ref["poses"][k].tobytes()
    for m in ref["points"]:
        assert got["points"][m].tobytes() == ref["points"][m].tobytes()

    def err(res):
        K, M = copy.deepcopy(kfs), copy.deepcopy(mps)
        O.apply_local_ba(K, M, res)
        d = [np.hypot(*(np.array(SC.project(np.asarray(K[k]["Tcw"], np.float64), np.asarray(M[m]["x3Dw"], np.float64))[:2]) - K[k]["un_xy"][sl])) for m in M for k, sl in M[m]["obs"].items()]
        assert all((k, m) not in planted for m in M for k in M[m]["obs"]) and all(K[k]["mp"][M[m]["obs"][k]] == m for m in M for k in M[m]["obs"])
        return float(np.mean(d))

    e_host = err(ref); e_dev = err(got)
    print("mean reprojection error of the kept observations after local BA:", e_dev)
    assert e_dev == e_host and e_host < 0.5 * np.sqrt(np.pi / 2)           # the mean distance of 0.5 px noise per axis from its centre (Rayleigh): 0.63 px
