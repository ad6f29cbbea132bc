"""GPU: sind_match_pnp_ransac (EPnP and CheckInliers of every sample of every candidate, and the Refine problems that follow from the counts, all on the device)
against the host library's entry points (sindh_pnp_*: the same source, csrc/host/epnp.hpp, compiled for the host) as bit patterns, and against the Python
restatement tests/pnp_ref.py.  The reference cannot be built for the tests (PnPsolver needs OpenCV), so parity is against the restatement, as for every matcher
call.  Then the error paths, the chain from descriptors to a pose on the synthetic stream, and the call on a handle shared with the other matcher calls."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
CAP = 192
RELOC = (0.99, 10, 300, 4, 0.5, 5.991)
SEED = 3                                                                # of the chain's random stream: with it the loop offers two poses that hold wrong matches before a clean one
KEYS = ("count", "bits", "R", "t", "refine", "refine_hyp", "refine_count", "refine_bits", "refine_R", "refine_t")


def _matcher(B, cap=CAP, K=None):
    import pnp_scene as S
    import sim3_scene as S3
    from sindslam_amd.matcher import ORBmatcher
    K = K or S.K
    return ORBmatcher(float(K[0]), float(K[1]), float(K[2]), float(K[3]), 40.0, (0, 640, 0, 480), S3.scale_factors(), nnratio=0.75, checkOri=True, cap=cap, max_batch=B)


def _assert_equal(got, ref, what):
    import pnp_cases as H
    for k in KEYS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        same = np.array_equal(H.bits64(g), H.bits64(r)) if g.dtype == np.float64 else np.array_equal(g, r)
        assert same, (what, k)


def _scene(sizes):
    """three candidates and 300 samples each, drawn without correspondence 4.  Candidate 0: correspondences 1, 3, 5, 7 are coplanar and sample 3 takes them.  Candidate 2:
    correspondences 2 and 6 are one and the same point and sample 4 takes both.  Candidate 1: correspondence 4 lies where sample 1's pose gives it depth exactly 0."""
    import pnp_cases as H
    import pnp_ref as P
    import pnp_scene as S
    from sindslam_amd import pnp
    rng = np.random.default_rng(sum(sizes))
    inps = [S.candidate(200 + n, n, outliers=0.3, noise=0.5) for n in sizes]
    sam = [np.stack([rng.choice(np.setdiff1d(np.arange(n), [4]), 4, replace=False) for _ in range(300)]).astype(np.int32) for n in sizes]
    c = inps[0]; X = c["x3Dw"].astype(np.float64)
    c["x3Dw"][7] = (X[1] + 0.3 * (X[3] - X[1]) + 0.6 * (X[5] - X[1])).astype(np.float32)
    Xc = c["x3Dw"][7].astype(np.float64) @ c["R"].T + c["t"]
    c["p2d"][7] = (S.K[2] + S.K[0] * Xc[0] / Xc[2], S.K[3] + S.K[1] * Xc[1] / Xc[2])
    sam[0][3] = (1, 3, 5, 7)
    c = inps[2]; c["x3Dw"][6] = c["x3Dw"][2]; c["p2d"][6] = c["p2d"][2]
    sam[2][4] = (2, 6, 8, 9)
    c = inps[1]; R, t, _ = H.host_pose(c["x3Dw"][sam[1][1]], c["p2d"][sam[1][1]], S.K)
    c["x3Dw"][4] = H.zero_depth_point(R, t)
    mins = [pnp.ransac_params(n, *RELOC[:5])[0] for n in sizes]
    return inps, sam, mins


@pytest.fixture(scope="module")
def matcher3():
    mt = _matcher(3)
    yield mt
    mt.close()


@pytest.mark.parametrize("sizes", [(15, 64, 65), (63, 129, CAP)])
def test_every_hypothesis_and_every_refine_equals_the_host_library_and_the_restatement(matcher3, sizes):
    import pnp_cases as H
    import pnp_ref as P
    import pnp_scene as S
    inps, sam, mins = _scene(sizes)
    host = H.host_evaluate(S.K)
    for n_its in (300, 65, 64, 5, 1):
        req = [(inp, s[:n_its], m, 0, None) for inp, s, m in zip(inps, sam, mins)]
        got = matcher3.PnPRansac(req); ref = host(req)
        for b in range(3):
            assert got[b]["bits"].shape == (n_its, (sizes[b] + 63) // 64)
            _assert_equal(got[b], ref[b], (n_its, b))
        if n_its == 300:
            full = got
    # the restatement: the first 8 hypotheses of each candidate and all its refines
    K = H.calib(S.K)
    for b, (inp, s, g) in enumerate(zip(inps, sam, full)):
        n = sizes[b]
        check = lambda R, t: P.check_inliers(inp["x3Dw"], inp["p2d"], inp["sigma2"], inp["th2"], *K, R, t)
        for h in range(8):
            R, t, _ = P.compute_pose(inp["x3Dw"][s[h]], inp["p2d"][s[h]], *K)
            inl, cnt = check(R, t)
            assert np.array_equal(H.bits64(g["R"][h]), H.bits64(np.array(R))) and np.array_equal(H.bits64(g["t"][h]), H.bits64(np.array(t))), (b, h)
            assert g["count"][h] == cnt and np.array_equal(g["bits"][h], P.pack_bits(inl)), (b, h)
        of_hyp, hyps = P.refine_plan(g["count"], mins[b], 0, False)
        assert list(g["refine"]) == of_hyp and list(g["refine_hyp"]) == hyps
        for r, h in enumerate(hyps):
            idx = np.flatnonzero(P.unpack_bits(g["bits"][h], n))
            R, t, _ = P.compute_pose(inp["x3Dw"][idx], inp["p2d"][idx], *K)
            inl, cnt = check(R, t)
            assert np.array_equal(H.bits64(g["refine_R"][r]), H.bits64(np.array(R))) and np.array_equal(H.bits64(g["refine_t"][r]), H.bits64(np.array(t))), (b, r)
            assert g["refine_count"][r] == cnt and np.array_equal(g["refine_bits"][r], P.pack_bits(inl)), (b, r)
    # what the scene claims
    R, t = full[1]["R"][1], full[1]["t"][1]; X = [float(v) for v in inps[1]["x3Dw"][4]]
    assert R[2][0] * X[0] + R[2][1] * X[1] + R[2][2] * X[2] + t[2] == 0 and not (int(full[1]["bits"][1][0]) >> 4) & 1
    assert sum(len(g["refine_hyp"]) > 0 for g in full) >= 2 and max(g["refine_count"].max() for g in full if len(g["refine_count"])) > sizes[1] // 2


def test_more_prefix_maxima_than_refine_slots_and_a_best_set_brought_in(matcher3):
    """samples sorted so that the counts ascend: every new count is a Refine problem, more than the 32 slots of a round.  Then the same samples in two calls, the
    second continuing from the best set of the first."""
    import pnp_cases as H
    import pnp_ref as P
    import pnp_scene as S
    inp = S.candidate(77, CAP, outliers=0.3, noise=1.0); other = S.candidate(78, 65, outliers=0.3, noise=1.0)
    rng = np.random.default_rng(1)
    draw = np.stack([rng.choice(CAP, 4, replace=False) for _ in range(900)]).astype(np.int32)
    cnt = np.array([H.host_check(inp, S.K, *H.host_pose(inp["x3Dw"][s], inp["p2d"][s], S.K)[:2])[0] for s in draw])
    order = np.argsort(cnt, kind="stable")[-300:]
    sam = draw[order]; asc = cnt[order]
    n_max = len(np.unique(asc[asc >= 10]))
    assert n_max > 32, "the scene is wrong: too few distinct counts"
    host = H.host_evaluate(S.K)
    sam2 = np.stack([rng.choice(65, 4, replace=False) for _ in range(40)]).astype(np.int32)
    req = [(inp, sam, 10, 0, None), (other, sam2, 10, 0, None)]
    got = matcher3.PnPRansac(req); ref = host(req)
    for b in range(2):
        _assert_equal(got[b], ref[b], ("ascending", b))
    assert len(got[0]["refine_hyp"]) == n_max and len(got[0]["refine_hyp"]) + len(got[1]["refine_hyp"]) > 32
    # two calls: the shuffled samples 0..149, then 150..299 from the best set so far
    sh = sam[rng.permutation(300)]
    whole, = matcher3.PnPRansac([(inp, sh, 10, 0, None)])
    first, = matcher3.PnPRansac([(inp, sh[:150], 10, 0, None)])
    best = int(np.argmax(first["count"]))                                # the first of the largest: the strict `>` keeps it
    bc, bb = int(first["count"][best]), first["bits"][best].copy()
    assert bc >= 10
    second, = matcher3.PnPRansac([(inp, sh[150:], 10, bc, bb)])
    _assert_equal(second, host([(inp, sh[150:], 10, bc, bb)])[0], "continued")
    assert -1 in list(second["refine_hyp"]) or second["count"].max() > bc or (second["count"] < 10).all()
    for part, off in ((first, 0), (second, 150)):
        for h in range(150):
            r, rw = int(part["refine"][h]), int(whole["refine"][off + h])
            assert (r < 0) == (rw < 0)
            if r >= 0:
                assert part["refine_count"][r] == whole["refine_count"][rw] and np.array_equal(part["refine_bits"][r], whole["refine_bits"][rw])
                assert np.array_equal(H.bits64(part["refine_R"][r]), H.bits64(whole["refine_R"][rw])) and np.array_equal(H.bits64(part["refine_t"][r]), H.bits64(whole["refine_t"][rw]))


def test_mixed_iteration_counts_and_an_empty_candidate(matcher3):
    import pnp_cases as H
    import pnp_scene as S
    inps, sam, mins = _scene((15, 64, 65))
    req = [(inps[0], sam[0][:7], mins[0], 0, None), (inps[1], sam[1][:0], mins[1], 0, None), (inps[2], sam[2][:130], mins[2], 0, None)]
    got = matcher3.PnPRansac(req); ref = H.host_evaluate(S.K)(req)
    assert len(got[1]["count"]) == 0 and len(got[1]["refine_hyp"]) == 0
    for b in (0, 2):
        _assert_equal(got[b], ref[b], b)


def test_errors_launch_nothing_and_leave_the_outputs():
    import pnp_scene as S
    from sindslam_amd import SindError
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import _PnpItem
    inp = S.candidate(7, 40); big = S.candidate(8, 70)
    sam = np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int32)
    mt = _matcher(2, cap=64)
    with pytest.raises(SindError, match="capacity"):
        mt.PnPRansac([(big, sam, 10, 0, None)])                          # 70 correspondences > cap 64
    with pytest.raises(SindError, match="max_batch"):
        mt.PnPRansac([(inp, sam, 10, 0, None)] * 3)
    with pytest.raises(SindError, match="sample index"):
        mt.PnPRansac([(inp, np.array([[0, 1, 2, 40]], np.int32), 10, 0, None)])
    with pytest.raises(SindError, match="repeats"):
        mt.PnPRansac([(inp, np.array([[0, 1, 2, 1]], np.int32), 10, 0, None)])
    with pytest.raises(SindError, match="sigma2"):
        mt.PnPRansac([(dict(inp, sigma2=-inp["sigma2"]), sam, 10, 0, None)])
    with pytest.raises(SindError, match="sigma2"):
        mt.PnPRansac([(dict(inp, sigma2=np.full(40, np.inf, np.float32)), sam, 10, 0, None)])
    with pytest.raises(SindError, match="min_inliers"):
        mt.PnPRansac([(inp, sam, 0, 0, None)])
    with pytest.raises(SindError, match="best_count"):
        mt.PnPRansac([(inp, sam, 10, 12, np.array([0xff], np.uint64))])  # 8 bits set, 12 claimed
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    a = dict(x3Dw=f32(big["x3Dw"]), p2d=f32(big["p2d"]), sigma2=f32(big["sigma2"]), samples=np.tile(sam, (200, 1)), count=np.full(400, 77, np.int32), inlier_bits=np.full(800, 77, np.uint64),
             R=np.full(3600, 77.0), t=np.full(1200, 77.0), refine=np.full(400, 77, np.int32), n_refines=np.full(1, 77, np.int32), refine_hyp=np.full(401, 77, np.int32),
             refine_count=np.full(401, 77, np.int32), refine_bits=np.full(802, 77, np.uint64), refine_R=np.full(3609, 77.0), refine_t=np.full(1203, 77.0))
    outs = ("count", "inlier_bits", "R", "t", "refine", "n_refines", "refine_hyp", "refine_count", "refine_bits", "refine_R", "refine_t")
    def call(n, n_its, B_=1, min_inliers=10, **change):
        q = (_PnpItem * 3)()
        for item in q:
            item.n, item.n_its, item.th2, item.min_inliers, item.best_count = n, n_its, 5.991, min_inliers, 0
            for k, v in a.items():
                setattr(item, k, None if change.get(k, 0) is None else change.get(k, v).ctypes.data)
        return lib().sind_match_pnp_ransac(mt._h, q, B_)
    untouched = lambda: all((a[k] == 77).all() for k in outs)
    assert call(65, 2) == SIND_E_CAPACITY and call(40, 301) == SIND_E_CAPACITY and call(40, 2, B_=3) == SIND_E_CAPACITY
    assert call(40, 2, samples=np.array([0, 1, 2, 3, -1, 5, 6, 7], np.int32)) == SIND_E_ARG and call(40, 2, samples=np.array([0, 1, 2, 3, 40, 5, 6, 7], np.int32)) == SIND_E_ARG
    assert call(40, 2, samples=np.array([0, 1, 2, 3, 5, 6, 7, 5], np.int32)) == SIND_E_ARG and call(40, 2, min_inliers=0) == SIND_E_ARG
    for k in ("x3Dw", "p2d", "sigma2", "samples", "count", "inlier_bits", "R", "refine", "n_refines", "refine_bits", "refine_t"):
        assert call(40, 2, **{k: None}) == SIND_E_ARG, k
    assert call(-1, 2) == SIND_E_ARG and call(40, -1) == SIND_E_ARG and lib().sind_match_pnp_ransac(mt._h, None, 1) == SIND_E_ARG
    assert untouched()
    assert call(40, 0) == 0 and call(0, 0, x3Dw=None, samples=None, count=None) == 0 and call(40, 2, B_=0) == 0 and lib().sind_match_pnp_ransac(mt._h, None, 0) == 0
    assert untouched()                                                   # n_its = 0 and B = 0 succeed and write nothing
    assert call(40, 2, B_=2) == 0 and (a["count"][:2] != 77).all() and (a["count"][2:] == 77).all() and (a["inlier_bits"][2:] == 77).all() and (a["t"][6:] == 77).all()      # the handle still works
    assert a["n_refines"][0] != 77
    mt.close()


@pytest.fixture(scope="module")
def chain(stream):
    """descriptors -> BowVector -> relocalisation candidates -> SearchByBoW -> PnPsolvers -> the loop of Tracking::Relocalization, on frames 5..8 of the synthetic stream as key
    frames and frame 9 as the lost frame, on a map without noise (pnp_scene.stream_candidate, ideal_map); twice on one handle that serves SearchByBoW in between, and once with the host library in the device's place"""
    import bow_scene as B
    import pnp_cases as H
    import pnp_scene as S
    from sindslam_amd import pnp
    from sindslam_amd.keyframe_db import KeyFrameDatabase
    from sindslam_amd.sim3 import Tape
    from sindslam_amd.vocabulary import ORBVocabulary
    kfs, lost = (5, 6, 7, 8), 9
    tree = B.stream_vocabulary(stream)
    voc = ORBVocabulary(tree, cap=4096, max_batch=5)
    tr = voc.transform_bow([B.stream_frame(stream, t)["desc"] for t in kfs + (lost,)], B.LEVELSUP)      # 1. sind_voc_transform_bow
    db = KeyFrameDatabase(8, cap_words=4096)
    for slot, (_, _, bw, bv) in enumerate(tr[:4]):
        db.add(slot, (bw, bv))
    cand = db.DetectRelocalizationCandidates((tr[4][2], tr[4][3]), {})   # 2. sind_bowdb_query and the tail; no covisibility graph: every key frame is its own group
    assert sorted(cand) == [0, 1, 2, 3] and cand[0] == 0                 # found: [0, 2, 3, 1], scores 0.78, 0.75, 0.76, 0.76
    K = tuple(float(c) for c in B.stream_frame(stream, lost)["cam"][:4])
    mt = _matcher(4, cap=4096, K=K)
    rng = np.random.default_rng(0)
    pairs = []
    for s in cand:
        f = B.stream_frame(stream, kfs[s])
        kf = dict(node=tr[s][0], valid=((f["depth"] > 0) & (rng.random(len(f["octave"])) > 0.15)).astype(np.uint8), angle=f["angle"], desc=f["desc"])
        pairs.append((kf, dict(node=tr[4][0], angle=B.stream_frame(stream, lost)["angle"], desc=B.stream_frame(stream, lost)["desc"])))
    matches = mt.SearchByBoW(pairs)                                      # 3. sind_match_by_bow, all candidates in one call
    inps = [None if n < 15 else S.stream_candidate(stream, kfs[s], lost, m, pairs[i][0]["valid"].astype(bool), ideal_map=True) for i, (s, (m, n)) in enumerate(zip(cand, matches))]
    assert sum(c is not None for c in inps) >= 2
    def accept(offered):
        """the caller's verdict in PoseOptimization's place, from the frame's own data: at least 50 inliers, and they reproject under the offered pose within a hundredth of a
        pixel (root mean square).  CheckInliers' bounds reach 77 px^2, so most poses PnPsolver offers hold wrong matches and are rejected; on the exact map a clean one passes"""
        def f(i, Tcw, vb, n):
            offered.append((i, Tcw.tobytes(), vb.tobytes(), n))
            c = inps[i]; sel = vb[c["indices"]]; T = Tcw.astype(np.float64)
            Pc = c["x3Dw"][sel].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            e2 = (K[2] + K[0] * Pc[:, 0] / Pc[:, 2] - c["p2d"][sel, 0]) ** 2 + (K[3] + K[1] * Pc[:, 1] / Pc[:, 2] - c["p2d"][sel, 1]) ** 2
            return n >= 50 and float(np.sqrt(e2.mean())) < 1e-2
        return f
    runs = []
    for _ in range(2):
        solvers = mt.pnp_solvers(inps, S.rand_stream(SEED))                 # 4. pnp_solvers and relocalization_pnp
        for s in solvers:
            if s is not None:
                s.SetRansacParameters(*RELOC)
        offered, trace = [], []
        runs.append((pnp.relocalization_pnp(solvers, accept(offered), trace=trace), offered, solvers, trace))
        again = mt.SearchByBoW(pairs)                                    # another kind of call on the same handle in between
        assert all(np.array_equal(a[0], m[0]) and a[1] == m[1] for a, m in zip(again, matches))
    ev = H.host_evaluate(K)

    def by_host_library(cands, acc):
        tape = Tape(S.rand_stream(SEED))
        solvers = [None if c is None else pnp.PnPsolver(ev, tape, c) for c in cands]
        for s in solvers:
            if s is not None:
                s.SetRansacParameters(*RELOC)
        offered, trace = [], []
        return pnp.relocalization_pnp(solvers, acc(offered), trace=trace), offered, solvers, trace
    by_host = by_host_library(inps, accept)
    # the same chain on the map as the key frames give it (their own back-projections, a median of 1 px off under the ground truth): the first pose rejected, then n >= 50
    raw = [None if c is None else S.stream_candidate(stream, kfs[s], lost, m, pairs[i][0]["valid"].astype(bool)) for i, (s, (m, n), c) in enumerate(zip(cand, matches, inps))]
    lenient = lambda offered: (lambda i, Tcw, vb, n: offered.append((i, Tcw.tobytes(), vb.tobytes(), n)) or (len(offered) > 1 and n >= 50))
    solvers = mt.pnp_solvers(raw, S.rand_stream(SEED))
    for s in solvers:
        if s is not None:
            s.SetRansacParameters(*RELOC)
    offered, trace = [], []
    raw_run = (pnp.relocalization_pnp(solvers, lenient(offered), trace=trace), offered, solvers, trace, by_host_library(raw, lenient), raw)
    mt.close(); voc.close(); db.close()
    return runs, by_host, B.stream_frame(stream, lost)["Tcw"].astype(np.float64), raw_run, K


def test_from_descriptors_to_a_pose_on_the_stream_on_a_shared_handle(chain):
    runs, by_host = chain[:2]
    for (res, offered, solvers, trace) in runs:
        assert trace == by_host[3]                                       # every iterate of the loop: candidate and bNoMore, so also the discard order
        assert offered == by_host[1] and len(offered) >= 3               # every pose offered to the caller, bit for bit, the rejected ones included
        assert res[0] == by_host[0][0] >= 0 and res[3] == by_host[0][3] and res[1].tobytes() == by_host[0][1].tobytes() and np.array_equal(res[2], by_host[0][2])
        assert res[2].sum() == solvers[res[0]].mnRefinedInliers >= 50


def test_the_chain_on_the_key_frames_own_map_equals_the_host_library(chain):
    """the map as the key frames give it: no pose from it can be exact (rehearsed: the accepted pose is 1.9e-2 / 5.7e-2 from the ground truth), but the loop on the device must
    offer what the loop on the host library offers, and the inliers of the accepted pose must be inliers by an FP64 computation of CheckInliers' test made here"""
    (res, offered, solvers, trace, host, raw), K = chain[3], chain[4]
    assert offered == host[1] and len(offered) >= 2 and trace == host[3]
    assert res[0] == host[0][0] >= 0 and res[3] == host[0][3] and res[1].tobytes() == host[0][1].tobytes() and np.array_equal(res[2], host[0][2])
    c = raw[res[0]]; sel = res[2][c["indices"]]; T = res[1].astype(np.float64)
    assert sel.sum() >= 50
    Pc = c["x3Dw"][sel].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    e2 = (K[2] + K[0] * Pc[:, 0] / Pc[:, 2] - c["p2d"][sel, 0]) ** 2 + (K[3] + K[1] * Pc[:, 1] / Pc[:, 2] - c["p2d"][sel, 1]) ** 2
    # the pose is mRefinedTcw, the FP32 of the FP64 pose the inliers were tested with: 1e-3 of the bound covers that rounding (some 1e-6 px on 3 m at 535 px focal length)
    assert (e2 < 5.991 * c["sigma2"][sel].astype(np.float64) * (1 + 1e-3)).all()


def test_the_pose_of_the_chain_meets_the_bound_of_the_cpu_test(chain):
    """The pose the chain ends with against the stream's ground truth, within the bound tests/test_pnp_cpu.py found on exact projections (|R - R_true| <= 1.938e-6,
    |t - t_true| <= 1.162e-5).  The chain's map is exact in the same sense (pnp_scene.stream_candidate, ideal_map): rightly matched map points lie on the rays of the
    frame's keypoints, wrong matches stay outliers (some 30 % of a candidate's matches).  With the map points left at the key frames' own back-projections, which
    reproject with a median error of 1 px under the ground truth itself, the same chain ends 1.9e-2 / 5.7e-2 away: that is the data's noise, not the solver's."""
    from pnp_cases import BOUND_R, BOUND_T
    runs, Tgt = chain[0], chain[2]
    Tcw = runs[0][0][1].astype(np.float64)
    dR, dt = np.abs(Tcw[:3, :3] - Tgt[:3, :3]).max(), np.abs(Tcw[:3, 3] - Tgt[:3, 3]).max()
    print(f"deviation from the stream's ground truth: rotation {dR:.3e}, translation {dt:.3e}; bounds {BOUND_R:.3e}, {BOUND_T:.3e}")
    assert dR <= BOUND_R and dt <= BOUND_T
