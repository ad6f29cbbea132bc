"""GPU: sind_match_sim3_optimize (Optimizer::OptimizeSim3 of every item in one launch, csrc/match_sim3opt.hip) against the host library's sindh_sim3_optimize (the same
source, csrc/host/sim3_opt.hpp, with the plain sequential loop) as bit patterns, every output; against the Python restatement tests/sim3opt_ref.py; the degenerate
scenes of the CPU test; independence of the items of a batch; the error paths; the call on a handle shared with other matcher calls; and LoopClosing::ComputeSim3 on
the synthetic stream, from SearchByBoW(KF, KF) to an accepted mScw, with the real matcher calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
CAP = 192
CHUNK = 64                                                              # edges per chunk of the kernel's ordered sum (SO_CHUNK of csrc/match_sim3opt.hip); a pair is two edges


def _matcher(B, cap=CAP, K=None):
    import poseopt_scene as P
    import sim3_scene as S3
    from sindslam_amd.matcher import ORBmatcher
    K = K or P.K5
    return ORBmatcher(float(K[0]), float(K[1]), float(K[2]), float(K[3]), P.BF, (0, 640, 0, 480), S3.scale_factors(), nnratio=0.75, checkOri=True, cap=cap, max_batch=B)


@pytest.fixture(scope="module")
def matcher3():
    mt = _matcher(3)
    yield mt
    mt.close()


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("sizes", [(10, (CHUNK - 2) // 2, CHUNK // 2), ((CHUNK + 2) // 2, CHUNK - 1, CHUNK), (CHUNK + 1, 2 * CHUNK + 1, CAP)])
def test_device_equals_the_host_library_bit_for_bit(matcher3, sizes, fix_scale):
    """pairs whose edges end two short of the chunk of the ordered sum, on it and two past it (31, 32, 33: also the sizes around half a wave), 10, sizes around two
    and four chunks, and the capacity; 30 % outliers, 0.5 px noise"""
    import sim3opt_scene as SC
    items = [SC.scene(300 + n + (7 if fix_scale else 0), n, outliers=0.3, noise=0.5, scale=1.0 if fix_scale else 1.07, start=(0.03, 0.03, 0.0 if fix_scale else 0.03)) for n in sizes]
    got = matcher3.OptimizeSim3(items, 10, fix_scale)
    ref = SC.HostOptimizer().OptimizeSim3(items, 10, fix_scale)
    for n, g, r in zip(sizes, got, ref):
        SC.assert_same(g, r, (n, fix_scale))
        assert g["n_stages"] >= 1 and g["n_bad"] <= int(g["removed"].sum()) and (g["n_stages"] == 1 or g["n_inliers"] == n - int(g["removed"].sum()))
    assert sum(g["n_stages"] == 2 for g in got) >= 2


@pytest.mark.parametrize("n", [10, 65])
def test_device_equals_the_restatement(matcher3, n):
    import sim3opt_ref as R
    import sim3opt_scene as SC
    s = SC.scene(n, n, outliers=0.2 if n > 10 else 0)
    for fix in (True, False):
        SC.assert_same(matcher3.OptimizeSim3([s], 10, fix)[0], R.optimize_sim3(s, 10, fix), (n, fix))


def test_degenerate_scenes_return_and_equal_the_host_library(matcher3):
    """a point at depth 0 (every step rejected), identical points (rank-deficient H), exact data at the identity (rho == 0 terminates); n = 0, n = 9 and 12 pairs with 3
    outliers return 0 with the input Sim3; a call in which every item returns early; an empty call"""
    import sim3opt_scene as SC
    host = SC.HostOptimizer()
    deg = SC.degenerates()
    early = [SC.scene(2, 0, outliers=0), SC.scene(9, 9, outliers=0), SC.scene(19, 12, outliers=3)]
    for fix in (True, False):
        for items in (list(deg.values()), early):
            got = matcher3.OptimizeSim3(items, 10, fix); ref = host.OptimizeSim3(items, 10, fix)
            for k, (g, r) in enumerate(zip(got, ref)):
                SC.assert_same(g, r, (fix, k))
    g = matcher3.OptimizeSim3(list(deg.values()), 10, True)
    assert np.isinf(g[0]["stage_chi2"]).all() and list(g[0]["stage_iters"]) == [5, 5] and list(g[2]["stage_iters"]) == [1, 1] and (g[2]["stage_chi2"] == 0).all()
    g = matcher3.OptimizeSim3(early, 10, True)
    for r, it in zip(g, early):
        n = len(it["inv_sigma2_1"])
        assert r["n_inliers"] == 0 and r["n_stages"] == (1 if n else 0) and np.array_equal(r["removed"].astype(bool), it["is_outlier"])
        h = SC.HostOptimizer().OptimizeSim3([dict(it, x3Dc1=it["x3Dc1"][:0], x3Dc2=it["x3Dc2"][:0], obs1_xy=it["obs1_xy"][:0], obs2_xy=it["obs2_xy"][:0], inv_sigma2_1=it["inv_sigma2_1"][:0],
                                                  inv_sigma2_2=it["inv_sigma2_2"][:0])])[0]      # the input Sim3 as the library converts it
        assert r["q"].tobytes() == h["q"].tobytes() and r["t"].tobytes() == h["t"].tobytes() and r["s"].tobytes() == np.float64(it["s12"]).tobytes()
    only_empty = matcher3.OptimizeSim3([early[0]] * 2, 10, True)              # a call of empty graphs launches nothing
    assert all(r["n_inliers"] == 0 and r["n_stages"] == 0 and r["s"] == np.float64(early[0]["s12"]) for r in only_empty)
    assert matcher3.OptimizeSim3([]) == []


def test_items_of_a_batch_are_independent(matcher3):
    import sim3opt_scene as SC
    items = [SC.scene(500 + n, n) for n in (40, 150, 77)]
    batch = matcher3.OptimizeSim3(items)
    for k, it in enumerate(items):
        SC.assert_same(matcher3.OptimizeSim3([it])[0], batch[k], k)
    swapped = matcher3.OptimizeSim3(items[::-1])[::-1]
    for k in range(3):
        SC.assert_same(swapped[k], batch[k], ("swapped", k))


def test_errors_launch_nothing_and_leave_the_outputs():
    import sim3opt_scene as SC
    from sindslam_amd import SindError
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import sim3opt_items
    import ctypes as C
    mt = _matcher(2, cap=64)
    ok, big = SC.scene(1, 40), SC.scene(2, 65)
    with pytest.raises(SindError, match="capacity"):
        mt.OptimizeSim3([big])                                           # 65 pairs > cap 64
    with pytest.raises(SindError, match="max_batch"):
        mt.OptimizeSim3([ok] * 3)
    with pytest.raises(SindError, match="inv_sigma2"):
        mt.OptimizeSim3([dict(ok, inv_sigma2_2=-ok["inv_sigma2_2"])])
    with pytest.raises(SindError, match="inv_sigma2"):
        mt.OptimizeSim3([dict(ok, inv_sigma2_1=np.where(np.arange(40) == 7, np.nan, ok["inv_sigma2_1"]))])
    for bad in (np.nan, np.inf):
        t = ok["t12"].copy(); t[1] = bad
        R = ok["R12"].copy(); R[1, 2] = bad
        for item in (dict(ok, t12=t), dict(ok, R12=R), dict(ok, s12=bad)):
            with pytest.raises(SindError, match="Sim3"):
                mt.OptimizeSim3([item])
        with pytest.raises(SindError, match="bad arguments"):
            mt.OptimizeSim3([ok], th2=bad)
    outs = ("q_out", "t_out", "s_out", "removed", "n_inliers", "n_bad", "n_stages", "stage_iters", "stage_chi2", "stage_lambda")
    fn = lib().sind_match_sim3_optimize

    def call(item, B=1, n=None, **null):
        arr, keep = sim3opt_items([item] * 3)
        for a in keep:
            for k in outs:
                a[k][...] = 77
        for q in arr:
            if n is not None:
                q.n = n
            for k in null:
                setattr(q, k, None)
        rc = fn(mt._h, arr, B, C.c_float(10.0), 1)
        return rc, [all((a[k] == 77).all() for k in outs) for a in keep], keep
    for rc, untouched, _ in (call(big), call(ok, B=3), call(ok, n=-1)):
        assert rc in (SIND_E_CAPACITY, SIND_E_ARG) and all(untouched)
    assert call(big)[0] == SIND_E_CAPACITY and call(ok, B=3)[0] == SIND_E_CAPACITY and call(ok, n=-1)[0] == SIND_E_ARG
    for k in ("x3Dc1", "x3Dc2", "obs1_xy", "obs2_xy", "inv_sigma2_1", "inv_sigma2_2", "K1", "K2", "R12", "t12", "q_out", "t_out", "s_out", "removed", "n_inliers"):
        rc, untouched, _ = call(ok, **{k: None})
        assert rc == SIND_E_ARG and all(untouched), k
    rc, untouched, _ = call(ok, B=2, inv_sigma2_1=None)                  # an error in any item: nothing written for any
    assert rc == SIND_E_ARG and all(untouched)
    assert fn(mt._h, None, 1, C.c_float(10.0), 1) == SIND_E_ARG and fn(mt._h, None, 0, C.c_float(10.0), 1) == 0
    rc, untouched, _ = call(ok, B=0)
    assert rc == 0 and all(untouched)
    rc, untouched, keep = call(ok, n=0, x3Dc1=None, x3Dc2=None, obs1_xy=None, obs2_xy=None, inv_sigma2_1=None, inv_sigma2_2=None, removed=None)      # n = 0 is valid: the empty graph
    assert rc == 0 and keep[0]["n_inliers"][0] == 0 and keep[0]["n_stages"][0] == 0 and keep[0]["s_out"][0] == np.float64(ok["s12"]) and (keep[0]["removed"] == 77).all() and untouched[1]
    rc, untouched, keep = call(ok, B=2, n_bad=None, n_stages=None, stage_iters=None, stage_chi2=None, stage_lambda=None)      # the diagnostics may be NULL; the handle still works
    ref = SC.HostOptimizer().OptimizeSim3([ok])[0]
    assert rc == 0 and untouched == [False, False, True]
    assert keep[0]["q_out"].tobytes() == ref["q"].tobytes() and np.array_equal(keep[1]["removed"], ref["removed"]) and keep[1]["n_inliers"][0] == ref["n_inliers"] and (keep[0]["stage_chi2"] == 77).all()
    mt.close()


# ---------------------------------------------------------------- on the synthetic stream: a shared handle, and LoopClosing::ComputeSim3 from SearchByBoW(KF, KF) to mScw
FEW, OBS_NOISE = 120, 6.0                                               # the chain's first candidate: 120 map points, keypoints 6 px off them.  Its map is consistent in 3-D, so the Sim3Solver offers a Sim3; OptimizeSim3 compares with the keypoints and keeps fewer than 20
SEED = 9                                                                # of the chain's random stream
RECOVERY_BOUND = 10 * 1.10e-7                                           # test_sim3opt_cpu.py: ten times the worst noise-free recovery measured there


def _stream_matcher(stream, B):
    import bow_scene as BS
    import match_scene as M
    from sindslam_amd.matcher import ORBmatcher
    cam = BS.stream_frame(stream, 9)["cam"]
    return ORBmatcher(float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), float(cam[4]), cam[6:10], M._scale_factors(), nnratio=0.75, checkOri=True, cap=4096, max_batch=B, cap_points=8192)


@pytest.fixture(scope="module")
def key_frames(stream):
    """frame 9 as mpCurrentKF; frames 6 (few map points, noisy keypoints), 8 (the loop key frame) and 7 (its covisible) in a map that has drifted rigidly; and frames 9 and 8
    on a map that is exact for each other"""
    import pnp_scene as S
    import sim3opt_scene as SC
    rigid = S.pose(np.random.default_rng(5), 0.05, 0.1)
    cur = SC.stream_key_frame(stream, 9, 0)
    few = SC.stream_key_frame(stream, 6, 1, rigid=rigid, few=FEW, obs_noise=OBS_NOISE)
    loop = SC.stream_key_frame(stream, 8, 2, rigid=rigid)
    cov = SC.stream_key_frame(stream, 7, 3, rigid=rigid)
    cur_i, loop_i, pairs = SC.ideal_pair(cur, loop)
    assert len(pairs) >= 200
    return dict(cur=cur, few=few, loop=loop, cov=cov, cur_i=cur_i, loop_i=loop_i)


def _compute_sim3(mt, optimizer, cur, cands, cov, fix=True):
    """LoopClosing::ComputeSim3 with real calls: SearchByBoWKF for the candidates, their Sim3Solvers, compute_sim3 with compute_sim3_accept (SearchBySim3, OptimizeSim3 on
    `optimizer`), loop_accept (SearchByProjectionSim3).  -> dict of everything the chain produced"""
    import sim3_scene as S3
    import sim3opt_scene as SC
    from sindslam_amd.optimizer import compute_sim3_accept, loop_accept
    from sindslam_amd.sim3 import compute_sim3
    matches = mt.SearchByBoWKF([(cur, c) for c in cands])
    inps = [None if n < 20 else SC.sim3_solver_input(cur, c, m) for c, (m, n) in zip(cands, matches)]      # :267-277
    solvers = mt.sim3_solvers(inps, fix, S3.rand_from(S3.raw_values(SEED)))
    trace = []
    accept = compute_sim3_accept(mt, cur, [dict(kf=c, match12=m) for c, (m, _) in zip(cands, matches)], solvers, fix, optimizer=optimizer, trace=trace)
    i, Scm, vb, discarded = compute_sim3(solvers, accept)
    out = dict(nmatches=[n for _, n in matches], matched=i, trace=trace, discarded=discarded, state=accept.state)
    if i >= 0:
        st = accept.state
        ids = np.where(st["vpMatches"] >= 0, cands[i]["mp"][np.maximum(st["vpMatches"], 0)], -1)              # mvpCurrentMatchedPoints
        out["loop"] = loop_accept(mt, cur, st["Scw"], [cov, cands[i]], ids)
    return out


@pytest.fixture(scope="module")
def chain(stream, key_frames):
    import sim3opt_scene as SC
    k = key_frames
    mt = _stream_matcher(stream, 2)
    on_device = _compute_sim3(mt, mt, k["cur"], [k["few"], k["loop"]], k["cov"])
    on_host = _compute_sim3(mt, SC.HostOptimizer(), k["cur"], [k["few"], k["loop"]], k["cov"])
    exact = _compute_sim3(mt, mt, k["cur_i"], [k["loop_i"]], k["cov"])
    mt.close()
    return on_device, on_host, exact


def test_the_chain_accepts_the_true_loop_key_frame_after_rejecting_the_first_candidate(chain, key_frames):
    """Candidate 0 is offered by its Sim3Solver (its map is consistent in 3-D), searched, optimised and rejected with fewer than 20 inliers (measured: 12 of 49
    pairs); the RANSAC schedule is planned again, candidate 1, the loop key frame, is accepted, and the projection of the loop map points
    finds far more than 40 matches."""
    d = chain[0]
    print("trace:", d["trace"], "nmatches:", d["nmatches"])
    steps = [(s[0], s[1]) for s in d["trace"]]
    assert steps == [("search_by_sim3", 0), ("optimize_sim3", 0), ("search_by_sim3", 1), ("optimize_sim3", 1)]
    assert d["trace"][1][2] < 20 <= d["trace"][3][2] and d["matched"] == 1 and min(d["nmatches"]) >= 20
    ok, total, matched, ids = d["loop"]
    assert ok and total >= 40 and total > int((d["state"]["vpMatches"] >= 0).sum())
    Scw = d["state"]["Scw"].astype(np.float64)                          # on the key frames' own maps, which are about a pixel off under the ground truth itself: printed, not bounded
    import sim3opt_scene as SC
    print("deviation of mScw from the ground truth on the key frames' own maps:", np.abs(Scw - SC.true_scw(key_frames["cur"], key_frames["loop"])).max())


def test_the_chain_equals_the_chain_with_the_host_twin(chain):
    d, h, _ = chain
    assert d["trace"] == h["trace"] and d["matched"] == h["matched"] and d["discarded"] == h["discarded"] and d["nmatches"] == h["nmatches"]
    for k in ("q", "t", "s"):
        assert np.asarray(d["state"]["S12"][k]).tobytes() == np.asarray(h["state"]["S12"][k]).tobytes(), k
    assert d["state"]["Scw"].tobytes() == h["state"]["Scw"].tobytes() and np.array_equal(d["state"]["vpMatches"], h["state"]["vpMatches"])
    assert d["loop"][:2] == h["loop"][:2] and np.array_equal(d["loop"][2], h["loop"][2]) and np.array_equal(d["loop"][3], h["loop"][3])


def test_the_chain_recovers_scw_where_the_map_is_exact(chain, key_frames):
    """frames 9 and 8 on a map that is exact for each other (sim3opt_scene.ideal_pair): rightly matched pairs have error 0 under the true Sim3 up to the FP32 rounding
    of the points, wrongly matched ones are more than 12 px off.  mbFixScale, as the RGB-D system runs.  Measured: 5.3e-8, 119 inliers of 119 pairs"""
    import sim3opt_scene as SC
    e = chain[2]
    assert e["matched"] == 0 and e["loop"][0]
    dev = np.abs(e["state"]["Scw"].astype(np.float64) - SC.true_scw(key_frames["cur_i"], key_frames["loop_i"])).max()
    print("deviation of mScw from the ground truth on the exact map:", dev, "inliers:", e["trace"])
    assert dev <= RECOVERY_BOUND
    assert np.float64(e["state"]["S12"]["s"]).tobytes() == np.float64(1.0).tobytes()


def test_on_a_handle_shared_with_the_loop_closers_searches(stream, key_frames):
    """SearchByBoWKF, OptimizeSim3, SearchBySim3, OptimizeSim3 again, PoseOptimization and SearchByBoWKF again one after the other on one handle give what each gives on a fresh one"""
    import poseopt_scene as P
    import sim3opt_scene as SC
    from sindslam_amd.optimizer import _sim3_side, sim3_item
    cur, loop = key_frames["cur"], key_frames["loop"]
    T1, T2 = cur["Tcw"].astype(np.float64), loop["Tcw"].astype(np.float64)
    R12 = (T1[:3, :3] @ T2[:3, :3].T).astype(np.float32); t12 = (T1[:3, 3] - R12.astype(np.float64) @ T2[:3, 3]).astype(np.float32)
    pose_item = P.scene(12, 150, "mixed")
    none1, none2 = np.zeros(len(cur["mp"]), bool), np.zeros(len(loop["mp"]), bool)

    def calls(mts):
        (m, n), = mts[0].SearchByBoWKF([(cur, loop)])
        item, idx = sim3_item(cur, loop, m, 1.0, R12, t12)
        a = mts[1].OptimizeSim3([item], 10, True)[0]
        b = mts[2].SearchBySim3([(cur["Tcw"], loop["Tcw"], 1.0, R12, t12, _sim3_side(cur, none1), _sim3_side(loop, none2))], 7.5)[0]
        c = mts[1].OptimizeSim3([item], 10, False)[0]
        d = mts[3].PoseOptimization([pose_item])[0]
        e = mts[1].OptimizeSim3([item], 10, True)[0]
        (m2, n2), = mts[0].SearchByBoWKF([(cur, loop)])
        assert np.array_equal(m, m2) and n == n2
        return (m, n), a, b, c, d, e, item
    shared = _stream_matcher(stream, 1)
    on_shared = calls([shared] * 4)
    fresh = [_stream_matcher(stream, 1) for _ in range(4)]
    on_fresh = calls(fresh)
    assert np.array_equal(on_shared[0][0], on_fresh[0][0]) and on_shared[0][1] == on_fresh[0][1] >= 100
    for k in (1, 3, 5):
        SC.assert_same(on_shared[k], on_fresh[k], k)
    SC.assert_same(on_shared[1], on_shared[5], "repeat")
    assert np.array_equal(on_shared[2][0], on_fresh[2][0]) and on_shared[2][1] == on_fresh[2][1] > 100
    P.assert_same(on_shared[4], on_fresh[4], "PoseOptimization")
    host = SC.HostOptimizer()
    SC.assert_same(on_shared[1], host.OptimizeSim3([on_shared[6]], 10, True)[0], "host"); SC.assert_same(on_shared[3], host.OptimizeSim3([on_shared[6]], 10, False)[0], "host, scale free")
    assert on_shared[1]["n_inliers"] >= 100 and len(on_shared[6]["inv_sigma2_1"]) > 2 * CHUNK
    for m in [shared] + fresh:
        m.close()
