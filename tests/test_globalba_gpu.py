"""GPU: sind_match_global_ba (Optimizer::BundleAdjustment as kernels per phase over the whole grid, csrc/match_globalba.hip) against the host library's sindh_global_ba
(the same source, csrc/host/global_ba.hpp, with the plain runner) as bit patterns, every output and diagnostic; against the parent's kernel (k_local_ba, stage 1) on
all-stereo scenes; against the Python restatement tests/globalba_ref.py; batches, the workspace's growth, the error paths and the limits; the call on a handle shared with
other matcher calls; and CorrectLoop followed by the global BA on a small synthetic map through sindslam_amd.optimizer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
T = 256                                                                 # GBA_THREADS of csrc/match.hpp: the lanes of a workgroup, one element each
GBA_MAX_KF = 4096


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


def _same(mt, items, what, iterations=10, robust=False):
    import globalba_scene as G
    got = mt.GlobalBundleAdjustment(items, iterations, robust); ref = G.HostGBA().GlobalBundleAdjustment(items, iterations, robust)
    for k, (g, r) in enumerate(zip(got, ref)):
        G.assert_same(g, r, (what, k))
    return got


@pytest.mark.parametrize("n_pts", [T - 1, T, T + 1])
def test_tail_workgroup_of_each_phase(matcher4, n_pts):
    """One free pose (key frame index 1) sees every point, so its edge list, the point count and its diagonal pair list sit one below, at and one above T = 256 on the
    same edges; a second free pose and the fixed one see a window.  Every phase is `one element per lane, if (idx < n)`: what can go wrong with size is the last
    workgroup."""
    import globalba_scene as G
    s = G.band_map(1000 + n_pts, 3, n_pts, 3, 1, kind="mixed", outliers=5, all_seen_by=1)
    g = _same(matcher4, [s], ("tail", n_pts), 10, True)[0]
    assert g["n_iters"] >= 3 and g["n_active_poses"] == 2 and int((np.asarray(s["obs_kf"]) == 1).sum()) == n_pts


@pytest.mark.parametrize("P", [1, 2, 10, 11, 42, 43])
def test_reduced_system_around_the_lane_counts(matcher4, P):
    """6 P = 6, 12, 60, 66 (crossing 64), 252, 258 (crossing T = 256): the one-workgroup solves, the per-column launches and the entries of x"""
    import globalba_scene as G
    s = G.band_map(2000 + P, P + 1, 6 * (P + 1), 4, 3, kind="stereo")
    g = _same(matcher4, [s], ("P", P), 10, False)[0]
    assert g["n_active_poses"] == P and g["n_iters"] >= 2 and g["solver_fail"] == 0


def test_block_columns_with_an_empty_a_short_and_a_full_envelope_row(matcher4):
    import globalba_scene as G
    s = G.band_map(31, 40, 160, 5, 3, loops=((2, 37),), kind="mixed", outliers=6)
    g = _same(matcher4, [s], "loop", 10, True)[0]
    assert g["env_entries"] < g["env_dense_entries"] and g["n_active_poses"] == 39


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_kinds_kernels_and_iteration_counts(matcher4, kind):
    import globalba_scene as G
    seed = {"mono": 100, "stereo": 200, "mixed": 300}[kind]
    for robust in (False, True):
        s = G.band_map(seed + robust, 7, 70, 4, 3, kind=kind, outliers=6)
        for iterations in (0, 1, 10, 20):
            g = _same(matcher4, [s], (kind, robust, iterations), iterations, robust)[0]
            assert g["n_iters"] <= iterations and (g["n_iters"] > 0) == (iterations > 0)


def test_one_larger_scene(matcher4):
    """43 key frames, 1 100 points x 4 observations"""
    import globalba_scene as G
    s = G.band_map(400, 43, 1100, 8, 4, loops=((1, 40),), kind="mixed", outliers=40)
    g = _same(matcher4, [s], "large", 10, True)[0]
    assert len(s["obs_kf"]) == 4406 and g["n_iters"] >= 3
    launches, waits = matcher4.global_ba_counts()
    print("larger scene: launches", launches, "host waits", waits, "iterations", g["n_iters"], "envelope", g["env_entries"], "of", g["env_dense_entries"])
    assert waits <= 2 + g["n_iters"] * 11                             # one per linearisation, at most ten trials each, the download


@pytest.mark.parametrize("seed,n_local,id0", [(41, 5, True), (42, 4, False)])
def test_against_the_parents_kernel(matcher4, seed, n_local, id0):
    """all-stereo, key frames of kinds 0 and 1 only: global BA at iterations = 5 with kernels is local BA's stage 1 (do_more = 0), the grid against one workgroup"""
    import globalba_scene as G
    import localba_scene as SC
    s = dict(SC.scene(seed, n_local, 0, 60, kind="stereo", outliers=5, obs_per_point=3, id0=id0), do_more=False)
    it, order = G.from_local(s)
    loc = matcher4.LocalBundleAdjustment([s])[0]
    g = matcher4.GlobalBundleAdjustment([it], 5, True)[0]
    assert np.array_equal(SC.bits(g["Tcw"]), SC.bits(loc["Tcw"][order])) and np.array_equal(SC.bits(g["x3Dw"]), SC.bits(loc["x3Dw"]))
    assert g["n_iters"] == loc["stage_iters"][0] and SC.bits(np.float64(g["chi2"])) == SC.bits(np.float64(loc["stage_chi2"][0]))


def test_device_equals_the_restatement(matcher4):
    import globalba_ref as R
    import globalba_scene as G
    s = G.band_map(2, 5, 24, 3, 3, kind="mixed", outliers=3)
    G.assert_same(matcher4.GlobalBundleAdjustment([s], 10, True)[0], R.global_ba(s, G.K5, 10, True), "restatement", keys=[k for k in G.OUTPUTS if not k.startswith("env")])


def test_batches_independence_and_growth(matcher4):
    import globalba_scene as G
    a = G.band_map(501, 4, 20, 3, 3, kind="mixed", outliers=2); b = G.band_map(502, 9, 70, 4, 3, kind="stereo", outliers=5); c = G.band_map(503, 3, 33, 3, 2, kind="mono", first_id=5)
    alone = matcher4.GlobalBundleAdjustment([a], 10, True)[0]
    for items, k in (([a, b, c], 0), ([b, a], 1), ([c, b, a, c], 2), ([a, a], 1)):
        G.assert_same(matcher4.GlobalBundleAdjustment(items, 10, True)[k], alone, ("neighbours", len(items), k))
    big = G.band_map(504, 12, 900, 5, 4, kind="mixed", outliers=30)
    _same(matcher4, [big, b], "grown", 10, True)
    G.assert_same(matcher4.GlobalBundleAdjustment([a], 10, True)[0], alone, "after the growth")
    assert matcher4.GlobalBundleAdjustment([]) == []


def test_literal_cases_equal_the_host_library(matcher4):
    """only key frame 0 (no active pose); no observations; no points; no fixed key frame; a point without observations and a free key frame without an edge"""
    import globalba_scene as G
    base = G.band_map(11, 4, 14, 4, 3, kind="mixed")
    only0 = G.band_map(12, 1, 9, 1, 1, kind="stereo")
    none = dict(base, obs_start=np.zeros(len(base["mp_id"]) + 1, np.int32), obs_kf=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32), u_right=np.zeros(0, np.float32), inv_sigma2=np.zeros(0, np.float32))
    nomp = dict(none, mp_id=np.zeros(0, np.int64), x3Dw=np.zeros((0, 3), np.float32), obs_start=np.zeros(1, np.int32))
    got = _same(matcher4, [only0, none, nomp], "literal", 10, True)
    assert got[0]["n_active_poses"] == 0 and got[0]["n_iters"] > 0 and got[1]["n_iters"] == -1 and got[2]["n_iters"] == -1 and not got[1]["included"].any()
    holes = G.without_kf_obs(G.without_point_obs(base, 3), 2)
    got = _same(matcher4, [G.band_map(13, 4, 14, 4, 3, kind="mixed", first_id=3), holes], "literal 2", 10, False)
    assert got[0]["n_active_poses"] == 4 and got[1]["n_active_poses"] == 2 and got[1]["included"][3] == 0 and got[1]["included"].sum() == 13


def test_error_paths_launch_nothing_and_leave_the_outputs_untouched(matcher4):
    import globalba_scene as G
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import globalba_items
    good = G.band_map(601, 4, 8, 4, 3, kind="mixed")
    for name, bad in G.bad_items().items():
        arr, keep = globalba_items([good, bad])
        for a in keep:
            a["Tcw_out"][:] = 7.0; a["x3Dw_out"][:] = 7.0; a["included"][:] = 7; a["n_iters"][:] = 7
        assert lib().sind_match_global_ba(matcher4._h, arr, 2, 10, 0) == SIND_E_ARG, name
        for a in keep:
            assert (a["Tcw_out"] == 7.0).all() and (a["x3Dw_out"] == 7.0).all() and (a["included"] == 7).all() and a["n_iters"][0] == 7, name
    arr, keep = globalba_items([good])
    assert lib().sind_match_global_ba(matcher4._h, None, 1, 10, 0) == SIND_E_ARG and lib().sind_match_global_ba(matcher4._h, arr, -1, 10, 0) == SIND_E_ARG
    assert lib().sind_match_global_ba(matcher4._h, arr, 1, -1, 0) == SIND_E_ARG
    arr, keep = globalba_items([good] * 5)
    assert lib().sind_match_global_ba(matcher4._h, arr, 5, 10, 0) == SIND_E_CAPACITY                # max_batch is 4
    many = G.band_map(602, GBA_MAX_KF + 1, 2, 2, 2, kind="mono")                                    # one key frame beyond the limit
    arr, keep = globalba_items([good, many])
    keep[0]["Tcw_out"][:] = 7.0
    assert lib().sind_match_global_ba(matcher4._h, arr, 2, 10, 0) == SIND_E_CAPACITY
    assert (keep[0]["Tcw_out"] == 7.0).all()
    _same(matcher4, [good], "after the errors")


def test_call_on_a_handle_shared_with_other_matcher_calls(matcher4):
    """one PoseOptimization before and one after, with unchanged results"""
    import globalba_scene as G
    import poseopt_scene as P
    s = P.scene(5, 60)
    before = matcher4.PoseOptimization([s])[0]
    a = G.band_map(701, 6, 40, 4, 3, kind="mixed", outliers=4)
    _same(matcher4, [a], "shared", 10, True)
    after = matcher4.PoseOptimization([s])[0]
    for k in ("Tcw", "outlier", "round_chi2", "round_lambda", "round_pose"):
        assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k
    _same(matcher4, [a], "shared, again", 10, True)


def _observed(kfs, mps):
    """the keypoints of essgraph_scene.toy_map's key frames: every slot sees its point where the (self-consistent, drifted) map projects it, all stereo, one level; a
    point closer than 0.5 m to a neighbour's image plane gets a keypoint at the image centre with weight 0"""
    import localba_scene as SC
    for k, kf in kfs.items():
        n = len(kf["mp"]); kf["un_xy"] = np.zeros((n, 2), np.float32); kf["u_right"] = np.zeros(n, np.float32); kf["inv_sigma2"] = np.ones(n, np.float32)
        for sl, m in enumerate(kf["mp"].tolist()):
            u, v, r, z = SC.project(np.asarray(kf["Tcw"], np.float64), np.asarray(mps[m]["x3Dw"], np.float64))
            if z > 0.5:
                kf["un_xy"][sl] = (u, v); kf["u_right"][sl] = r
            else:
                kf["un_xy"][sl] = (320.0, 240.0); kf["u_right"][sl] = 300.0; kf["inv_sigma2"][sl] = 0.0


def test_correct_loop_then_global_ba_end_to_end(matcher4):
    """optimizer.correct_loop and then optimizer.run_global_bundle_adjustment on the toy map, once over the device calls and once over the host library: the same collected
    item, the same result bits, the same map"""
    import copy

    import essgraph_scene as S
    import globalba_scene as G
    from sindslam_amd import optimizer as OPT

    class Host(S.HostEss, G.HostGBA):
        pass

    kfs, mps, cur, loop, Scw, matched, _ = S.toy_map()
    _observed(kfs, mps)
    kfs_h, mps_h = copy.deepcopy(kfs), copy.deepcopy(mps)
    tr, tr_h = {}, {}
    OPT.correct_loop(matcher4, kfs, mps, cur, loop, Scw, matched, True)
    OPT.correct_loop(Host(), kfs_h, mps_h, cur, loop, Scw, matched, True)
    r = OPT.run_global_bundle_adjustment(matcher4, kfs, mps, cur, [0], trace=tr)
    r_h = OPT.run_global_bundle_adjustment(Host(), kfs_h, mps_h, cur, [0], trace=tr_h)
    assert all(np.array_equal(tr["item"][k], tr_h["item"][k]) for k in tr["item"]) and r_h["n_iters"] >= 2 and r_h["solver_fail"] == 0 and r_h["n_active_poses"] == len(kfs) - 1
    G.assert_same(r, r_h, "global BA after correct_loop")
    assert all(np.array_equal(kfs[k]["Tcw"], kfs_h[k]["Tcw"]) and np.array_equal(kfs[k]["TcwBefGBA"], kfs_h[k]["TcwBefGBA"]) for k in kfs)
    assert all(np.array_equal(mps[m]["x3Dw"], mps_h[m]["x3Dw"]) for m in mps)
