"""GPU: the five searches of one ORBmatcher handle, interleaved.  The handle shares its staging between the kinds of call (the flags of the acting side
hold valid|has_obs, kf_valid or has_mp1; the taken array of the searched side holds cur_taken or has_mp2), so every call here finds staging left
behind by a different kind, by a larger batch or by a longer frame, and must still equal the restatement its own test file uses (oracle_lib,
localmap_ref, bow_ref).  All equalities; floats are compared as uint32 bit patterns.  The "plenty of matches" guards are half of what the restatement
finds on these scenes (the found values stand beside them).  The last test does the same for the two graph optimizers, which pack their items into streams
of the handle that grow between calls, against their host twins."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NNRATIO = 0.8


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_frustum(got, fr):
    assert np.array_equal(got["in_view"], fr["in_view"])
    assert np.array_equal(got["level"], fr["level"])
    assert np.array_equal(_bits(got["proj_xyr"]), _bits(fr["proj_xyr"]))
    assert np.array_equal(_bits(got["view_cos"]), _bits(fr["view_cos"]))
    assert got["n_to_match"] == fr["n_to_match"]


def test_five_searches_interleaved_on_one_handle():
    import bow_ref as W
    import bow_scene as B
    import localmap_ref as R
    import localmap_scene as L
    import match_scene as S
    import oracle_lib as O
    from sindslam_amd.matcher import ORBmatcher

    cam, sc, Tc, Tl, last, cur = S.stress_pair(5)
    lcam, lsc, lTc, mp, lcur = L.stress_local_map(5)
    tris = [B.tri_special_pair(0), B.tri_special_pair(2, n=100)]
    for c, s in [(lcam, lsc)] + [(t[0], t[1]) for t in tris]:                    # one camera, one set of scale factors: one handle serves every scene
        assert np.array_equal(c, cam) and np.array_equal(s, sc)
    assert np.array_equal(lTc, Tc) and all(np.array_equal(lcur[k], cur[k]) for k in cur)
    kf, bcur = B.bow_stress_pair(4)
    few_kf = {k: v[:65] for k, v in kf.items()}
    few = {k: v[:500] for k, v in mp.items()}
    cur_free = {k: v for k, v in cur.items() if k != "taken"}
    slots = dict(x3Dw=mp["x3Dw"], max_dist=mp["max_dist"], min_dist=mp["min_dist"], valid=mp["flags"] & 1, angle=np.zeros(len(mp["flags"]), np.float32), desc=mp["desc"])
    cur_kf = dict(cur); cur_kf["angle"] = np.zeros(len(cur["octave"]), np.float32)

    # the restatements, each computed once
    tri_ref = [W.search_for_triangulation(c, s, T2, Cw1, F12, k1, k2, 0, True) for c, s, T2, Cw1, F12, k1, k2 in tris]
    proj_free = O.search_by_projection(cam, sc, Tc, Tl, last, cur_free, 15.0)
    proj_taken = O.search_by_projection(cam, sc, Tc, Tl, last, cur, 15.0)
    assert (proj_free[0] != proj_taken[0]).sum() > 121, "the scene is wrong, not the matcher"      # found: 242 keypoints tell a leaked `taken` from zeros
    bow_full = W.search_by_bow(kf, bcur, 0.75, True)
    bow_few = W.search_by_bow(few_kf, bcur, 0.75, True)
    fr_full, fr_few = R.frustum(cam, sc, Tc, mp), R.frustum(cam, sc, Tc, few)
    loc_full = R.search_local(cam, sc, mp, cur, fr_full, 3.0, NNRATIO)
    loc_few = R.search_local(cam, sc, few, cur, fr_few, 3.0, NNRATIO)
    kf_ref = R.search_kf(cam, sc, Tc, slots, cur_kf, 10.0, 100, True)

    def local_equals(g, fr, ref):
        _assert_frustum(g, fr)
        assert g["nmatches"] == ref[1] and np.array_equal(g["match_of_cur"], ref[0])

    mt = ORBmatcher(cam[0], cam[1], cam[2], cam[3], cam[4], cam[6:10], sc, nnratio=NNRATIO, checkOri=True, cap=4096, max_batch=2, cap_points=3000)

    # 1. triangulation, B = 2: has_mp2 goes into the shared taken array, has_mp1 into the shared flags
    got = mt.SearchForTriangulation([t[2:] for t in tris])
    for (m12, nm, pairs), (mo, no, po), least in zip(got, tri_ref, (97, 41)):    # found: 194, 82
        assert nm == no and np.array_equal(m12, mo) and pairs.tolist() == [list(p) for p in po]
        assert nm > least

    # 2. projection, B = 1, no `taken`: a NULL cur_taken reads as zeros, not as what step 1 left
    (m, n), = mt.SearchByProjection([(Tc, Tl, last, cur_free)], 15.0)
    assert n == proj_free[1] and np.array_equal(m, proj_free[0])
    assert n > 201                                                               # found: 403 (394 with `taken`)

    # 3. BoW, B = 2, then B = 1 with a shorter key-frame side
    got = mt.SearchByBoW([(kf, bcur), (kf, bcur)], nnratio=0.75)
    for m, n in got:
        assert n == bow_full[1] and np.array_equal(m, bow_full[0])
        assert n > 30                                                            # found: 60
    (m, n), = mt.SearchByBoW([(few_kf, bcur)], nnratio=0.75)
    assert n == bow_few[1] and np.array_equal(m, bow_few[0])
    assert n > 0                                                                 # found: 7

    # 4. local map, B = 2 (the full map and its first 500 points), then B = 1 on the 500 points alone
    got = mt.SearchLocalPoints([(Tc, mp, cur), (Tc, few, cur)], 3.0)
    local_equals(got[0], fr_full, loc_full); local_equals(got[1], fr_few, loc_few)
    assert got[0]["nmatches"] > 263 and got[1]["nmatches"] > 47                  # found: 527, 95
    got, = mt.SearchLocalPoints([(Tc, few, cur)], 3.0)
    local_equals(got, fr_few, loc_few)

    # 5. relocalisation search over the same map points as a key frame's slots
    (m, n), = mt.SearchByProjectionKF([(Tc, slots, cur_kf)], 10.0, 100)
    assert n == kf_ref[1] and np.array_equal(m, kf_ref[0])
    assert n > 466                                                               # found: 932

    # 6. projection again, with `taken`
    (m, n), = mt.SearchByProjection([(Tc, Tl, last, cur)], 15.0)
    assert n == proj_taken[1] and np.array_equal(m, proj_taken[0])
    assert n > 197                                                               # found: 394
    assert mt.last_rounds() >= 2

    # 7. BoW once more, the full pair
    (m, n), = mt.SearchByBoW([(kf, bcur)], nnratio=0.75)
    assert n == bow_full[1] and np.array_equal(m, bow_full[0])
    mt.close()


def test_local_ba_and_essential_graph_alternate_on_one_handle_with_items_of_changing_size():
    """The two graph optimizers pack their items one after the other into streams that grow between calls (csrc/match_handle.hpp: PackedItems), each call kind its own.
    On one handle: a small item, a larger one (the streams grow), a batch of two unequal items (the second item's offsets are not the first's), the small one again
    (nothing of the larger calls is read).  Every output of every call equals the host twin's bit for bit.  The scenes are checked on the host first: both stages of
    local BA run with planted outliers erased, the essential graph iterates and its factorisation never fails."""
    import essgraph_scene as E
    import localba_scene as LB
    from sindslam_amd.matcher import ORBmatcher

    lb = {"small": LB.scene(61, 2, 1, 6, kind="mixed", outliers=1), "big": LB.scene(61, 5, 3, 40, kind="mixed", outliers=3)}
    es = {"small": E.scene(61, 4, window=1, loop=1, n_mp=8), "big": E.scene(61, 12, window=3, loop=2, n_mp=40)}
    assert [len(es[k]["edge_i"]) for k in ("small", "big")] == [5, 38] and [len(lb[k]["obs_kf"]) for k in ("small", "big")] == [18, 320]
    lb_ref = {k: LB.HostBA().LocalBundleAdjustment([v], K=LB.K5)[0] for k, v in lb.items()}
    es_ref = {k: E.HostEss().OptimizeEssentialGraph([v], True)[0] for k, v in es.items()}
    for r in lb_ref.values():
        assert r["n_stages"] == 2 and min(r["stage_iters"]) >= 2 and r["erase"].sum() >= 1
    for r in es_ref.values():
        assert r["solver_fail"] == 0 and r["n_iters"] >= 2

    mt = ORBmatcher(*[float(k) for k in LB.K5], (0.0, 640.0, 0.0, 480.0), [1.2 ** k for k in range(8)], cap=512, max_batch=2)
    for step, (lb_names, es_names) in enumerate(((["small"], ["small"]), (["big"], ["big"]), (["small", "big"], ["big", "small"]), (["small"], ["small"]))):
        for k, g in zip(lb_names, mt.LocalBundleAdjustment([lb[k] for k in lb_names])):
            LB.assert_same(g, lb_ref[k], ("local BA", step, k))
        for k, g in zip(es_names, mt.OptimizeEssentialGraph([es[k] for k in es_names], True)):
            E.assert_same(g, es_ref[k], ("essential graph", step, k))
    mt.close()
