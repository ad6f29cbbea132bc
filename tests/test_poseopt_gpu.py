"""GPU: sind_match_pose_optimize (Optimizer::PoseOptimization of every item in one launch, csrc/match_pose.hip) against the host library's sindh_pose_optimize (the same
source, csrc/host/pose_opt.hpp, with the plain sequential loop) as bit patterns, every output; against the Python restatement tests/poseopt_ref.py; the degenerate
scenes of the CPU test; independence of the items of a batch; the error paths; the call on a handle shared with other matcher calls; and the relocalisation chain
on the synthetic stream, from descriptors to an accepted, optimised pose, with the real matcher calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
CAP = 192
RELOC = (0.99, 10, 300, 4, 0.5, 5.991)
SEED = 3                                                                # of the chain's random stream: with it the loop offers at least one pose that the chain rejects
FEW = 130                                                               # map points of the chain's first key frame: enough for PnPsolver to offer a pose, too few for the chain to accept it
KEEP = 0.15                                                             # the share of a key frame's map points that the chain's SearchByBoW is given; the projection searches reach all


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


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("sizes", [(3, 64, 65), (63, 129, CAP), (127, 128, 129)])
def test_device_equals_the_host_library_bit_for_bit(matcher3, sizes, kind):
    """sizes around the wave (64), the chunk of the ordered sum (128) and the capacity; 30 % outliers, 0.5 px noise"""
    import poseopt_scene as P
    items = [P.scene(300 + n + 7 * len(kind), n, kind, outliers=0.3, noise=0.5) for n in sizes]
    got = matcher3.PoseOptimization(items)
    ref = P.HostOptimizer().PoseOptimization(items)
    for n, g, r in zip(sizes, got, ref):
        P.assert_same(g, r, (n, kind))
        assert g["n_rounds"] == (4 if n >= 10 else 1) and g["n_good"] == n - int(g["outlier"].sum())


@pytest.mark.parametrize("n", [10, 65])
def test_device_equals_the_restatement(matcher3, n):
    import poseopt_ref as R
    import poseopt_scene as P
    s = P.scene(n, n, "mixed")
    P.assert_same(matcher3.PoseOptimization([s])[0], R.pose_optimization(s["x3Dw"], s["obs_xy"], s["u_right"], s["inv_sigma2"], s["Tcw"], P.K5), n)


def test_degenerate_scenes_return_and_equal_the_host_library(matcher3):
    """n = 2 (returns 0, pose untouched), n = 9 (one round), a point at depth 0 (NaN system: every step rejected), identical points (rank-deficient H), mono and stereo"""
    import poseopt_scene as P
    host = P.HostOptimizer()
    batches = [[P.scene(2, 2, "mixed", outliers=0), P.scene(9, 9, "mixed"), P.behind_camera()], [P.identical_points(), P.identical_points(stereo=True)]]
    for items in batches:
        got = matcher3.PoseOptimization(items); ref = host.PoseOptimization(items)
        for k, (g, r) in enumerate(zip(got, ref)):
            P.assert_same(g, r, k)
    g = matcher3.PoseOptimization(batches[0])
    assert g[0]["n_good"] == 0 and g[0]["n_rounds"] == 0 and g[0]["Tcw"].tobytes() == batches[0][0]["Tcw"].tobytes()
    assert g[1]["n_rounds"] == 1 and g[2]["n_rounds"] == 4 and np.isnan(g[2]["round_chi2"]).all() and np.isfinite(g[2]["Tcw"]).all()
    only_small = matcher3.PoseOptimization([batches[0][0]] * 2)            # a call in which no item reaches 3 correspondences launches nothing
    assert all(r["n_good"] == 0 and r["n_rounds"] == 0 for r in only_small)
    assert matcher3.PoseOptimization([]) == []


def test_items_of_a_batch_are_independent(matcher3):
    import poseopt_scene as P
    items = [P.scene(500 + n, n, "mixed") for n in (40, 150, 77)]
    batch = matcher3.PoseOptimization(items)
    for k, it in enumerate(items):
        P.assert_same(matcher3.PoseOptimization([it])[0], batch[k], k)
    swapped = matcher3.PoseOptimization(items[::-1])[::-1]
    for k in range(3):
        P.assert_same(swapped[k], batch[k], ("swapped", k))


def test_errors_launch_nothing_and_leave_the_outputs():
    import poseopt_scene as P
    from sindslam_amd import SindError
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import poseopt_items
    mt = _matcher(2, cap=64)
    ok, big = P.scene(1, 40), P.scene(2, 65)
    with pytest.raises(SindError, match="capacity"):
        mt.PoseOptimization([big])                                       # 65 correspondences > cap 64
    with pytest.raises(SindError, match="max_batch"):
        mt.PoseOptimization([ok] * 3)
    with pytest.raises(SindError, match="inv_sigma2"):
        mt.PoseOptimization([dict(ok, inv_sigma2=-ok["inv_sigma2"])])
    with pytest.raises(SindError, match="inv_sigma2"):
        mt.PoseOptimization([dict(ok, inv_sigma2=np.where(np.arange(40) == 7, np.nan, ok["inv_sigma2"]))])
    for bad in (np.nan, np.inf):
        T = ok["Tcw"].copy(); T[1, 3] = bad
        with pytest.raises(SindError, match="pose"):
            mt.PoseOptimization([dict(ok, Tcw=T)])
    outs = ("Tcw_out", "outlier", "n_good", "n_rounds", "round_iters", "round_nbad", "round_pose", "round_chi2", "round_lambda")

    def call(item, B=1, n=None, **null):
        arr, keep = poseopt_items([item] * 3)
        for a in keep:
            for k in outs:
                a[k][...] = 77
        for q in arr:
            if n is not None:
                q.n = n
            for k in null:
                setattr(q, k, None)
        rc = lib().sind_match_pose_optimize(mt._h, arr, B)
        return rc, [all((a[k] == 77).all() for k in outs) for a in keep], keep
    for rc, untouched, _ in (call(big), call(ok, B=3), call(ok, n=-1)):
        assert rc in (SIND_E_CAPACITY, SIND_E_ARG) and all(untouched)
    assert call(big)[0] == SIND_E_CAPACITY and call(ok, B=3)[0] == SIND_E_CAPACITY and call(ok, n=-1)[0] == SIND_E_ARG
    for k in ("x3Dw", "obs_xy", "u_right", "inv_sigma2", "Tcw", "Tcw_out", "outlier", "n_good", "n_rounds"):
        rc, untouched, _ = call(ok, **{k: None})
        assert rc == SIND_E_ARG and all(untouched), k
    rc, untouched, _ = call(ok, B=2, inv_sigma2=None)                     # an error in any item: nothing written for any
    assert rc == SIND_E_ARG and all(untouched)
    assert lib().sind_match_pose_optimize(mt._h, None, 1) == SIND_E_ARG and lib().sind_match_pose_optimize(mt._h, None, 0) == 0
    rc, untouched, _ = call(ok, B=0)
    assert rc == 0 and all(untouched)
    rc, untouched, keep = call(ok, n=0, x3Dw=None, obs_xy=None, u_right=None, inv_sigma2=None, outlier=None)      # n = 0 is valid: the reference's `return 0`
    assert rc == 0 and keep[0]["n_good"][0] == 0 and keep[0]["n_rounds"][0] == 0 and (keep[0]["Tcw_out"] == 77).all() and untouched[1]
    rc, untouched, keep = call(ok, B=2, round_iters=None, round_nbad=None, round_pose=None, round_chi2=None, round_lambda=None)      # the round arrays may be NULL; the handle still works
    ref = P.HostOptimizer().PoseOptimization([ok])[0]
    assert rc == 0 and untouched == [False, False, True]
    assert keep[0]["Tcw_out"].tobytes() == ref["Tcw"].tobytes() and np.array_equal(keep[1]["outlier"], ref["outlier"]) and keep[1]["n_good"][0] == ref["n_good"] and (keep[0]["round_pose"] == 77).all()
    mt.close()


def test_on_a_handle_shared_with_pnp_and_the_projection_search(stream):
    """PnPRansac, PoseOptimization, SearchByProjectionKF one after the other on one handle give what each gives on a fresh one"""
    import localmap_scene as L
    import pnp_scene as S
    import poseopt_scene as P
    cam, sc, Tc, kf, cur = L.reloc_pair(stream, 6)
    K = tuple(float(c) for c in cam[:4]) + (P.BF,)
    inp = S.candidate(11, 120); sam = np.stack([np.random.default_rng(k).choice(120, 4, replace=False) for k in range(40)]).astype(np.int32)
    item = P.scene(12, 150, "mixed")

    def calls(mts):
        a = mts[0].PnPRansac([(inp, sam, 10, 0, None)])[0]
        b = mts[1].PoseOptimization([item])[0]
        c = mts[2].SearchByProjectionKF([(Tc, kf, cur)], 10.0, 100)[0]
        d = mts[1].PoseOptimization([item])[0]
        return a, b, c, d
    shared = _matcher(1, cap=4096, K=K)
    on_shared = calls([shared] * 3)
    fresh = [_matcher(1, cap=4096, K=K) for _ in range(3)]
    on_fresh = calls(fresh)
    for k in ("count", "bits", "R", "t", "refine", "refine_count", "refine_R", "refine_t"):
        assert np.asarray(on_shared[0][k]).tobytes() == np.asarray(on_fresh[0][k]).tobytes(), k
    P.assert_same(on_shared[1], on_fresh[1], "PoseOptimization"); P.assert_same(on_shared[3], on_fresh[3], "PoseOptimization again"); P.assert_same(on_shared[3], on_shared[1], "repeat")
    assert np.array_equal(on_shared[2][0], on_fresh[2][0]) and on_shared[2][1] == on_fresh[2][1] > 0
    P.assert_same(on_shared[1], P.HostOptimizer(K).PoseOptimization([item])[0], "host")
    for m in [shared] + fresh:
        m.close()


def _chain_setup(stream, keep=None, few=None):
    """descriptors -> SearchByBoW against four key frames -> PnPsolvers -> the loop of Tracking::Relocalization with relocalization_accept (PoseOptimization and
    SearchByProjectionKF) on frames 5..8 of the synthetic stream as key frames and frame 9 as the lost frame, on the key frames' own map; once with the device's
    PoseOptimization, once with the host library's in the same chain"""
    import bow_scene as B
    import localmap_scene as L
    import match_scene as M
    import pnp_scene as S
    import poseopt_scene as P
    import sim3_scene as S3
    from sindslam_amd import pnp
    from sindslam_amd.optimizer import PoseOptimization, relocalization_accept
    from sindslam_amd.vocabulary import ORBVocabulary
    kfs, lost = (5, 6, 7, 8), 9
    voc = ORBVocabulary(B.stream_vocabulary(stream), cap=4096, max_batch=5)
    tr = voc.transform_bow([B.stream_frame(stream, t)["desc"] for t in kfs + (lost,)], B.LEVELSUP)
    F = B.stream_frame(stream, lost)
    K = tuple(float(c) for c in F["cam"][:4]) + (P.BF,)
    mt = _matcher(4, cap=4096, K=K)
    rng = np.random.default_rng(0)
    sc = M._scale_factors()
    pairs, slots = [], []
    for s, t in enumerate(kfs):
        f = B.stream_frame(stream, t)
        has_point = (f["depth"] > 0).astype(np.uint8)                      # every keypoint with a depth holds a map point: the slots SearchByProjection can reach
        valid = (has_point.astype(bool) & (rng.random(len(f["octave"])) < (keep or KEEP))).astype(np.uint8)      # the share of them that SearchByBoW is given
        if s == 0:                                                       # the first candidate is a key frame that holds few map points, all of them given to SearchByBoW
            has_point = has_point * 0; has_point[rng.permutation(np.nonzero(f["depth"] > 0)[0])[:(few or FEW)]] = 1; valid = has_point.copy()
        pairs.append((dict(node=tr[s][0], valid=valid, angle=f["angle"], desc=f["desc"]), dict(node=tr[4][0], angle=F["angle"], desc=F["desc"])))
        z = f["depth"].astype(np.float64); xy = f["un_xy"].astype(np.float64); cam = f["cam"]; T = f["Tcw"].astype(np.float64)
        Xc = np.stack([(xy[:, 0] - cam[2]) * z / cam[0], (xy[:, 1] - cam[3]) * z / cam[1], z], 1)
        Xw = ((Xc - T[:3, 3]) @ T[:3, :3]).astype(np.float32); Xw[z <= 0] = (0, 0, 1)
        mx, mn = L._invariance(np.linalg.norm(Xc, axis=1), f["octave"], sc)
        slots.append(dict(x3Dw=Xw, max_dist=mx, min_dist=mn, valid=has_point, angle=f["angle"], desc=f["desc"], mp=10000 * s + np.arange(len(z), dtype=np.int64)))
    matches = mt.SearchByBoW(pairs)
    inps, cands = [], []
    grid = M.stream_pair(stream, lost)[5]
    assert np.array_equal(grid["un_xy"], F["un_xy"])
    for s, (m, n) in enumerate(matches):
        inps.append(None if n < 15 else S.stream_candidate(stream, kfs[s], lost, m, pairs[s][0]["valid"].astype(bool)))
        cands.append(dict(match_mp=np.where(m >= 0, 10000 * s + m.astype(np.int64), -1), match_x3Dw=slots[s]["x3Dw"][np.maximum(m, 0)], kf=slots[s]))
    assert sum(c is not None for c in inps) >= 2

    def run(optimizer, seed=SEED):
        frame = dict(un_xy=F["un_xy"], u_right=F["u_right"], inv_sigma2=(np.float32(1.0) / S3.sigma2_of(F["octave"]).astype(np.float32)).astype(np.float32), octave=F["octave"], angle=F["angle"],
                     desc=F["desc"], grid_start=grid["grid_start"], grid_idx=grid["grid_idx"], mp=np.full(len(F["octave"]), -1, np.int64), x3Dw=np.zeros((len(F["octave"]), 3), np.float32),
                     Tcw=np.eye(4, dtype=np.float32))
        solvers = mt.pnp_solvers(inps, S.rand_stream(seed))
        for sv in solvers:
            if sv is not None:
                sv.SetRansacParameters(*RELOC)
        steps, offered = [], []
        inner = relocalization_accept(mt, frame, cands, optimize=lambda f: PoseOptimization(optimizer, f), trace=steps)

        def accept(i, Tcw, vb, n):
            v = inner(i, Tcw, vb, n); offered.append((i, Tcw.tobytes(), bool(v), frame["Tcw"].tobytes(), frame["mp"].tobytes()))
            return v
        res = pnp.relocalization_pnp(solvers, accept)
        return res, steps, offered, frame
    return run, mt, P.HostOptimizer(K), (lambda: (mt.close(), voc.close())), F["Tcw"].astype(np.float64)


@pytest.fixture(scope="module")
def chain(stream):
    run, mt, host, close, Tgt = _chain_setup(stream)
    on_device = run(mt)
    on_host = run(host)
    close()
    return on_device, on_host, Tgt


def test_the_chain_ends_in_an_accepted_optimised_pose(chain):
    (res, steps, offered, frame), _, Tgt = chain
    print("steps:", steps)
    assert res[0] >= 0 and offered[-1][2]
    nGood = [s for s in steps if s[0].startswith("optimize")][-1][1]
    assert nGood >= 50 and steps[-1] == ("verdict", True)
    assert int((frame["mp"] >= 0).sum()) >= 50
    T = frame["Tcw"].astype(np.float64)                                  # on the key frames' own map, which is about a pixel off under the ground truth itself: printed, not bounded
    print("deviation of the optimised pose from the ground truth:", np.abs(T - Tgt).max())


def test_the_chain_equals_the_chain_with_the_host_librarys_pose_optimization(chain):
    """The accepted candidate, its pose and every step of the chain equal those with the host library's PoseOptimization.  The first candidate is a key frame with
    FEW map points: PnPsolver offers a pose from it, the chain optimises it (nGood about 22), searches, optimises again (about 44), searches in the narrow window and
    rejects it; the second candidate starts below 50 as well and is accepted after the wide search and the second optimisation."""
    (res, steps, offered, frame), (hres, hsteps, hoffered, hframe), _ = chain
    assert steps == hsteps and offered == hoffered
    assert res[0] == hres[0] and res[1].tobytes() == hres[1].tobytes() and np.array_equal(res[2], hres[2]) and res[3] == hres[3]
    assert frame["Tcw"].tobytes() == hframe["Tcw"].tobytes() and np.array_equal(frame["mp"], hframe["mp"]) and np.array_equal(frame["outlier"], hframe["outlier"])
    assert sum(1 for o in hoffered if not o[2]) >= 1                     # the seed: at least one offered pose is rejected by the chain
    assert {"search1", "optimize2", "search2"} <= {st[0] for st in hsteps}      # and the real projection searches ran
