"""GPU: sind_match_sim3_ransac (Sim3Solver's ComputeSim3 on the host and CheckInliers for every hypothesis of every candidate in one launch) against the Python
restatement tests/sim3_ref.py: counts and inlier words equal, s12 / R12 / t12 as bit patterns (a NaN as a NaN).  The reference cannot be built for the tests
(Sim3Solver needs OpenCV), so parity is against the restatement, as for every matcher call.  Then the error paths, the whole chain from SearchByBoW(KF, KF) to a
Sim3 on key frames of the synthetic stream, and the call on a handle shared with the other matcher calls."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
CAP = 192


def bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _matcher(B, cap=CAP, K=None):
    import sim3_scene as S
    from sindslam_amd.matcher import ORBmatcher
    K = K or S.K
    return ORBmatcher(float(K[0]), float(K[1]), float(K[2]), float(K[3]), 40.0, (0, 640, 0, 480), S.scale_factors(), nnratio=0.75, checkOri=True, cap=cap, max_batch=B)


def _reference(inp, triples, fix):
    import sim3_ref as R
    rs = R.Solver(inp, fix, None)
    res = dict(count=[], bits=[], s12=[], R12=[], t12=[])
    for t in triples:
        h = rs.hypothesis(t); inl, cnt = R.check_inliers(rs.sv, h["T12"], h["T21"])
        res["count"].append(cnt); res["bits"].append(R.pack_bits(inl)); res["s12"].append(h["s12"]); res["R12"].append(h["R12"]); res["t12"].append(h["t12"])
    return {k: np.array(v) for k, v in res.items() if v}, rs


def _scene(sizes, fix):
    """three candidates and 300 triples each.  Candidate 0: correspondences 2, 5, 7 are one and the same pair of points, and iteration 3 samples them: a NaN hypothesis.
    Candidate 1 (pKF2 at the origin, so that x3Dw2 is the camera-frame point): correspondence 4 lies where iteration 1's T12 gives it z = 0 exactly."""
    import sim3_ref as R
    import sim3_scene as S
    rng = np.random.default_rng(sum(sizes) + fix)
    inps = [S.candidate(100 + n, n, s12=1.0 if fix else 1.15, T2w=np.eye(4) if b == 1 else None)[0] for b, n in enumerate(sizes)]
    tris = []
    for inp in inps:
        n = len(inp["sigma2_1"])
        tris.append(np.stack([rng.choice(np.setdiff1d(np.arange(n), [4]), 3, replace=False) for _ in range(300)]).astype(np.int32))
    for k in ("x3Dw1", "x3Dw2"):
        inps[0][k][5] = inps[0][k][2]; inps[0][k][7] = inps[0][k][2]
    tris[0][3] = (2, 5, 7)
    T12 = R.Solver(inps[1], fix, None).hypothesis(tris[1][1])["T12"]
    z = np.float32(-np.float64(T12[2, 3]) / np.float64(T12[2, 2])); found = None
    lo = hi = z
    for _ in range(400):
        for c in (lo, hi):
            if R.to_camera(T12, np.array([[0, 0, c]], np.float32))[0, 2] == 0:
                found = c
        if found is not None:
            break
        lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
    assert found is not None, "the scene is wrong: no float z with T12[2] . (0, 0, z, 1) == 0"
    inps[1]["x3Dw2"][4] = (0, 0, found)
    return inps, tris


@pytest.fixture(scope="module")
def matcher3():
    mt = _matcher(3)
    yield mt
    mt.close()


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("sizes", [(20, 64, 65), (63, 129, CAP)])
def test_every_hypothesis_equals_the_restatement(matcher3, sizes, fix):
    import sim3_ref as R
    inps, tris = _scene(sizes, fix)
    refs = [_reference(inp, t, fix) for inp, t in zip(inps, tris)]
    for n_its in (300, 5, 1):
        got = matcher3.Sim3Ransac([(inp, t[:n_its]) for inp, t in zip(inps, tris)], fix)
        for b, (g, (r, _)) in enumerate(zip(got, refs)):
            assert np.array_equal(g["count"], r["count"][:n_its]), (n_its, b)
            assert g["bits"].shape == (n_its, (sizes[b] + 63) // 64) and np.array_equal(g["bits"], r["bits"][:n_its]), (n_its, b)
            for k in ("s12", "R12", "t12"):
                assert np.array_equal(bits(g[k]), bits(r[k][:n_its])), (n_its, b, k)
    # what the scene claims
    r0, r1 = refs[0][0], refs[1][0]
    assert np.isnan(r0["R12"][3]).all() and r0["count"][3] == 0 and (r0["bits"][3] == 0).all()
    rs = refs[1][1]; T12 = R.compute_sim3(*[[[X[tris[1][1][c]][r] for c in range(3)] for r in range(3)] for X in (rs.sv["X3Dc1"], rs.sv["X3Dc2"])], fix)["T12"]
    assert R.to_camera(T12, rs.sv["X3Dc2"][4:5])[0, 2] == 0 and not (int(r1["bits"][1][0]) >> 4) & 1
    assert max(r["count"].max() for r, _ in refs) > sizes[0] // 2 and min(r["count"].min() for r, _ in refs) == 0      # hypotheses with many inliers and with none
    if not fix:
        assert (r1["count"] > 20).sum() > 40                             # found: 81 / 101 of the 300 samples would make iterate return


def test_mixed_iteration_counts_and_an_empty_candidate(matcher3):
    inps, tris = _scene((20, 64, 65), False)
    ref = [_reference(inp, t[:k], False)[0] for inp, t, k in zip(inps, tris, (7, 0, 130))]
    got = matcher3.Sim3Ransac([(inps[0], tris[0][:7]), (inps[1], tris[1][:0]), (inps[2], tris[2][:130])], False)
    assert len(got[1]["count"]) == 0
    for b in (0, 2):
        assert np.array_equal(got[b]["count"], ref[b]["count"]) and np.array_equal(got[b]["bits"], ref[b]["bits"]) and np.array_equal(bits(got[b]["t12"]), bits(ref[b]["t12"]))


def test_errors_launch_nothing_and_leave_the_outputs():
    import sim3_scene as S
    from sindslam_amd import SindError
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import _Sim3Item
    inp = S.candidate(7, 40)[0]; big = S.candidate(8, 70)[0]
    tri = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    mt = _matcher(2, cap=64)
    with pytest.raises(SindError, match="capacity"):
        mt.Sim3Ransac([(big, tri)], False)                               # 70 correspondences > cap 64
    with pytest.raises(SindError, match="max_batch"):
        mt.Sim3Ransac([(inp, tri)] * 3, False)
    with pytest.raises(SindError, match="triple index"):
        mt.Sim3Ransac([(inp, np.array([[0, 1, 40]], np.int32))], False)
    with pytest.raises(SindError, match="sigma2"):
        mt.Sim3Ransac([(dict(inp, sigma2_1=-inp["sigma2_1"]), tri)], False)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    a = dict(T1w=f32(inp["T1w"]), T2w=f32(inp["T2w"]), x3Dw1=f32(big["x3Dw1"]), x3Dw2=f32(big["x3Dw2"]), sigma2_1=f32(big["sigma2_1"]), sigma2_2=f32(big["sigma2_2"]),
             triple=np.tile(tri, (200, 1)), count=np.full(400, 77, np.int32), inlier_bits=np.full(800, 77, np.uint64), s12=np.full(400, 77, np.float32), R12=np.full(3600, 77, np.float32),
             t12=np.full(1200, 77, np.float32))
    def call(n, n_its, B_=1, **change):
        q = (_Sim3Item * 3)()
        for item in q:
            item.n, item.n_its = n, n_its
            for k, v in a.items():
                setattr(item, k, None if change.get(k, 0) is None else change.get(k, v).ctypes.data)
        return lib().sind_match_sim3_ransac(mt._h, q, B_, 0)
    untouched = lambda: all((a[k] == 77).all() for k in ("count", "inlier_bits", "s12", "R12", "t12"))
    assert call(65, 2) == SIND_E_CAPACITY and call(40, 301) == SIND_E_CAPACITY and call(40, 2, B_=3) == SIND_E_CAPACITY
    assert call(40, 2, triple=np.array([0, 1, 2, 3, -1, 5], np.int32)) == SIND_E_ARG and call(40, 2, triple=np.array([0, 1, 2, 3, 40, 5], np.int32)) == SIND_E_ARG
    for k in ("T1w", "x3Dw2", "sigma2_1", "triple", "count", "inlier_bits", "R12"):
        assert call(40, 2, **{k: None}) == SIND_E_ARG, k
    assert call(-1, 2) == SIND_E_ARG and call(40, -1) == SIND_E_ARG and lib().sind_match_sim3_ransac(mt._h, None, 1, 0) == SIND_E_ARG
    assert untouched()
    assert call(40, 0) == 0 and call(0, 0, x3Dw1=None, triple=None, count=None) == 0 and call(40, 2, B_=0) == 0 and lib().sind_match_sim3_ransac(mt._h, None, 0, 0) == 0
    assert untouched()                                                   # n_its = 0 and B = 0 succeed and write nothing
    assert call(40, 2, B_=2) == 0 and (a["count"][:2] != 77).all() and (a["count"][2:] == 77).all() and (a["inlier_bits"][2:] == 77).all() and (a["t12"][6:] == 77).all()      # the handle still works
    mt.close()


def test_from_bow_matches_to_a_sim3_on_stream_key_frames_and_on_a_shared_handle(stream):
    """SearchByBoW(KF, KF) for three candidates, their Sim3Solvers, the loop of LoopClosing::ComputeSim3 with a toy accept; before and after, the same handle serves
    SearchByBoWKF, and a second run of the whole loop gives the same answer."""
    import bow_scene as B
    import loop_ref as L
    import loop_scene as LS
    import sim3_ref as R
    import sim3_scene as S
    from sindslam_amd.sim3 import compute_sim3
    k1 = LS.kf_stream_pair(stream, 9, 5, seed=0)[0]
    pairs = [(k1, LS.kf_stream_pair(stream, 9, t, seed=t)[1]) for t in (6, 7, 8)]
    K = tuple(float(c) for c in B.stream_frame(stream, 9)["cam"][:4])
    mt = _matcher(3, cap=4096, K=K)
    matches = mt.SearchByBoWKF(pairs)
    inps = [S.stream_candidate(stream, 9, t, m) for t, (m, _) in zip((6, 7, 8), matches)]
    assert [len(c["indices1"]) for c in inps] == [n for _, n in matches] and min(n for _, n in matches) > 130
    toy = lambda i, Scm, vb: vb.sum() >= 200                             # "OptimizeSim3 keeps enough": rejects the first returns
    raw = S.raw_values(9)
    rand = S.rand_from(raw)
    ref = R.compute_sim3_loop([R.Solver(c, False, rand) for c in inps], toy)
    outs = []
    for _ in range(2):
        solvers = mt.sim3_solvers(inps, False, S.rand_from(raw))
        outs.append(compute_sim3(solvers, toy) + (solvers,))
        again = mt.SearchByBoWKF(pairs)                                  # another kind of call on the same handle in between
        assert all(np.array_equal(a[0], m[0]) and a[1] == m[1] for a, m in zip(again, matches))
    for i, Scm, vb, disc, solvers in outs:
        assert i == ref[0] and i >= 0 and np.array_equal(bits(Scm), bits(ref[1])) and np.array_equal(vb, ref[2]) and disc == ref[3]
        s = solvers[i]
        assert vb.sum() == s.mnBestInliers >= 100                        # found: 200 of 331 on candidate 2, after the returns of candidates 0 (158) and 1 (169) were rejected
        assert abs(float(s.GetEstimatedScale()) - 1 / 1.08) < 0.05 and np.array_equal(bits(s.GetEstimatedScale() * s.GetEstimatedRotation() + np.float32(0)), bits(Scm[:3, :3]))
        assert np.array_equal(bits(s.GetEstimatedTranslation()), bits(Scm[:3, 3]))
    (m, nm), = mt.SearchByBoWKF(pairs[:1])
    mo, no, _ = L.search_by_bow_kf(*pairs[0], 0.75, True)
    assert nm == no and np.array_equal(m, mo)
    mt.close()
