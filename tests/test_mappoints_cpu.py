"""CPU: the host twins sindh_triangulate and sindh_update_points (csrc/host/map_points.hpp, the source the kernels of csrc/match_mappoints.hip compile too) against the
Python restatement tests/mappoints_ref.py, bit for bit, on random scenes and on the literal cases; the triangulated points against NumPy's FP64 SVD of the same A
(plausibility, not parity); the error paths; sindslam_amd.mapping on a toy map against the literal per-neighbour loop; and a sanitizer build of the twins as a program of
its own.  The measured figure named below is in profiles/match_map_points.txt."""
import os
import subprocess

import numpy as np
import pytest

SIND_E_ARG = -1
SVD_SEEDS = range(100, 120)
SVD_DEVIATION = 2.11e-6                                                   # measured over SVD_SEEDS: the largest |x3D - FP64 LAPACK's| / |FP64 LAPACK's|; asserted times four


@pytest.fixture(scope="module")
def H():
    import mappoints_scene as SC
    return SC.HostMap()


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_triangulation_twin_equals_the_restatement_on_random_scenes(H, kind):
    import mappoints_ref as R
    import mappoints_scene as SC
    seed = {"mono": 1, "stereo": 2, "mixed": 3}[kind]
    pairs = [SC.tri_scene(10 * seed + k, n, kind, baseline=b) for k, (n, b) in enumerate(((40, None), (25, 0.02), (30, 0.3), (0, None)))]
    got = H.Triangulate(pairs); ref = R.triangulate(pairs, SC.K5, SC.SCALE)
    seen = set()
    for k, (g, r) in enumerate(zip(got, ref)):
        SC.assert_same(g, r, SC.TRI_OUT, (kind, k))
        assert g["nnew"] == int((g["status"] == 0).sum()) and ((g["status"] == -1) == (pairs[k]["match12"] < 0)).all()
        seen |= set(zip(g["how"].tolist(), g["status"].tolist()))
    assert (0, 0) in seen and (kind == "mono" or (1, 0) in seen or (2, 0) in seen)
    assert H.Triangulate([]) == []


def test_triangulation_literal_cases(H):
    """one case per status code and per `how`, each rejected by the named test alone: the expected status and how are the scene's, not the twin's"""
    import mappoints_ref as R
    import mappoints_scene as SC
    cases = SC.tri_literal_cases()
    assert {st for _, st, _ in cases.values()} == set(range(9)) and {h for _, _, h in cases.values()} == {-1, 0, 1, 2}
    for name, (pair, status, how) in cases.items():
        g = H.Triangulate([pair])[0]; r = R.triangulate([pair], SC.K5, SC.SCALE)[0]
        SC.assert_same(g, r, SC.TRI_OUT, name)
        assert (g["status"][0], g["how"][0], g["nnew"]) == (status, how, int(status == 0)), (name, g)
    a, b = SC.cos_rays(cases["cos_just_below_0.9998"][0]), SC.cos_rays(cases["cos_just_above_0.9998"][0])
    assert np.float64(a) < 0.9998 <= np.float64(b) and b - a <= 4 * np.spacing(np.float32(0.9998)), (a, b)
    g = H.Triangulate([cases[n][0] for n in cases])                      # and all of them as one batch
    assert [int(x["status"][0]) for x in g] == [st for _, st, _ in cases.values()]


def test_triangulated_points_agree_with_an_fp64_svd(H):
    """well-conditioned scenes (baseline 0.1 to 0.5 m, depth 1 to 4 m, 0.5 px noise): x3D of the twin's FP32 Jacobi SVD against numpy.linalg.svd of the same A in FP64.
    The two differ by rounding alone; the bound is four times the largest deviation measured over these seeds (2.11e-6, profiles/match_map_points.txt)."""
    import mappoints_ref as R
    import mappoints_scene as SC
    c = R.camera(SC.K5, SC.SCALE)
    worst, count = 0.0, 0
    for seed in SVD_SEEDS:
        p = SC.tri_scene(seed, 60, "mono", wrong=0, unmatched=0)
        g = H.Triangulate([p])[0]
        T = lambda k: [[np.float32(v) for v in row] for row in np.asarray(p[k], np.float32)]
        for i, j in enumerate(p["match12"]):
            if g["how"][i] != 0 or g["status"][i] == 2:
                continue
            A = np.array(R.triangulation_matrix(c, T("Tcw1"), T("Tcw2"), p["kf1"]["un_xy"][i], p["kf2"]["un_xy"][j])[2], np.float64)
            v = np.linalg.svd(A)[2][3]; X = v[:3] / v[3]
            worst = max(worst, float(np.linalg.norm(g["x3D"][i].astype(np.float64) - X) / np.linalg.norm(X))); count += 1
    print("largest relative deviation of x3D from the FP64 SVD over", count, "points:", worst)
    assert count >= 1000 and worst <= 4 * SVD_DEVIATION


def test_update_twin_equals_the_restatement_on_random_scenes(H):
    import mappoints_ref as R
    import mappoints_scene as SC
    items = [SC.mp_scene(1, [1, 2, 3, 5, 8, 13, 0, 4, 7, 6]), SC.mp_scene(2, [63, 64, 65, 130]), SC.mp_scene(3, [2] * 20 + [6] * 20, bad=0.6), SC.mp_scene(4, [3, 4, 5], flags=(True, False)),
             SC.mp_scene(5, [3, 4, 5], flags=(False, True)), SC.mp_scene(6, [])]
    got = H.UpdateMapPoints(items); ref = R.update_points(items, SC.SCALE)
    for k, (g, r) in enumerate(zip(got, ref)):
        SC.assert_same(g, r, SC.MP_OUT, k)
    assert (got[3]["normal"] == 7.0).all() and (got[3]["updated"] == 0).all() and (got[4]["desc"] == 0xAB).all() and (got[4]["best_obs"] == -1).all()      # the flag that is off leaves its outputs
    assert (got[2]["best_obs"] == -1).any() and (got[2]["best_obs"] >= 0).any()
    assert H.UpdateMapPoints([]) == []


def test_update_literal_cases(H):
    """the expected winners are worked out by hand in the scene (descriptors on a line: distance = difference of positions)"""
    import mappoints_ref as R
    import mappoints_scene as SC
    for name, (item, best) in SC.mp_literal_cases().items():
        g = H.UpdateMapPoints([item])[0]; r = R.update_points([item], SC.SCALE)[0]
        SC.assert_same(g, r, SC.MP_OUT, name)
        assert g["best_obs"].tolist() == best, (name, g["best_obs"])
        for j, b in enumerate(best):
            a = item["obs_start"][j]
            assert (g["desc"][j] == (item["obs_desc"][a + b] if b >= 0 else 0xAB)).all(), (name, j)
    it, _ = SC.mp_literal_cases()["normal_cases"]
    g = H.UpdateMapPoints([it])[0]
    assert g["updated"].tolist() == [1, 1, 1, 1]                         # a point whose only observer is bad still gets its normal: bad key frames count
    X = it["x3Dw"].astype(np.float64); Ow = it["Ow"].astype(np.float64)
    d = lambda j, k: np.linalg.norm(X[j] - Ow[k])
    top = len(SC.SCALE) - 1
    for j, (kf, octave) in enumerate(((0, 0), (1, top), (3, top), (3, top))):      # the reference key frame first, in the middle, last; octave 0 and nlevels - 1
        assert abs(g["max_dist"][j] - d(j, kf) * SC.SCALE[octave]) <= 1e-5 * g["max_dist"][j] and abs(g["min_dist"][j] * SC.SCALE[top] - g["max_dist"][j]) <= 1e-5 * g["max_dist"][j]
    n3 = sum((X[0] - Ow[k]) / d(0, k) for k in (0, 1, 2)) / 3            # the bad key frame 1 counted in the sum and in n
    assert np.abs(g["normal"][0] - n3).max() < 1e-6 and np.abs(g["normal"][0] - sum((X[0] - Ow[k]) / d(0, k) for k in (0, 2)) / 2).max() > 1e-3


def test_error_paths_write_nothing(H):
    import mappoints_scene as SC
    from sindslam_amd.matcher import mappoints_items, triangulate_items
    for name, bad in SC.mp_bad_items().items():
        arr, keep = mappoints_items([SC.mp_scene(32, [2, 3]), bad])
        assert SC.host().sindh_update_points(arr, 2, SC.SCALE.ctypes.data, len(SC.SCALE)) == SIND_E_ARG, name
        for a in keep:
            assert (a["desc_out"] == 0xAB).all() and (a["best_obs"] == -1).all() and (a["normal_out"] == 7.0).all() and (a["max_dist"] == 7.0).all() and (a["updated"] == 0).all(), name
    for name, bad in SC.tri_bad_pairs().items():
        arr, keep = triangulate_items([SC.tri_scene(42, 9), bad])
        for a in keep:
            a["x3D"][:] = 7.0; a["status"][:] = 77; a["nnew"][:] = 77
        assert SC.host().sindh_triangulate(arr, 2, SC.K5.ctypes.data, SC.SCALE.ctypes.data, len(SC.SCALE)) == SIND_E_ARG, name
        for a in keep:
            assert (a["x3D"] == 7.0).all() and (a["status"] == 77).all() and a["nnew"][0] == 77, name
    ok = SC.mp_bad_items()["ref_obs -1 with observations and do_normal"]; ok["do_normal"] = False      # without the normal nothing reads the reference key frame
    assert H.UpdateMapPoints([ok])[0]["best_obs"][2] >= 0


def test_create_new_map_points_equals_the_literal_loop(H):
    """mapping.create_new_map_points (all searches in one call on the key frame as it was, one Triangulate, the replay, one update) against CreateNewMapPoints as the
    reference runs it: neighbour after neighbour with refreshed slots, every point updated at once.  The toy map makes the difference matter: every point that waits for
    triangulation is seen by all four neighbours, so the batched searches return it up to four times."""
    import copy

    import mappoints_scene as SC
    from sindslam_amd import mapping as M
    kfs, mps, cur = SC.toy_map(5)
    assert len(M.neighbours_for_triangulation(H, cur, kfs)) == len(kfs) - 2      # the key frame 0.03 m away fails the baseline test
    ka, ma = copy.deepcopy(kfs), copy.deepcopy(mps); kb, mb = copy.deepcopy(kfs), copy.deepcopy(mps)
    new = M.create_new_map_points(H, cur, ka, ma)
    lit = SC.literal_create_new_map_points(H, cur, kb, mb)
    assert new == lit and len(new) >= 60
    SC.same_maps((ka, ma), (kb, mb))
    second = [next(k for k in ma[m]["obs"] if k != cur) for m in new]      # the neighbour a point was created for
    kept = M.neighbours_for_triangulation(H, cur, kfs)
    assert second == sorted(second, key=kept.index) and second.count(kept[0]) >= 30 and len(set(second)) >= 2      # (neighbour, idx1) order; later neighbours add what the first did not see
    waiting = {int(p) for sl, p in enumerate(kfs[cur]["point_of_slot"]) if kfs[cur]["mp"][sl] < 0}
    assert len(new) <= len(waiting)                                      # one point per waiting slot at most, though every neighbour's search returned it again
    for m in new:
        p = ma[m]
        assert p["ref_kf"] == cur and len(p["obs"]) == 2 and p["desc"].shape == (32,) and np.isfinite(p["normal"]).all() and 0 < p["min_dist"] < p["max_dist"]
        truth = [kfs[k]["point_of_slot"][sl] for k, sl in p["obs"].items()]
        assert truth[0] == truth[1]                                      # both keypoints are the same scene point
    assert H.checkOri is False


def test_point_updates_of_the_call_sites(H):
    """process_new_keyframe_points, update_after_fuse and the three update_after_* of optimizer.py pass the right point sets"""
    import copy

    import mappoints_scene as SC
    from sindslam_amd import mapping as M
    from sindslam_amd import optimizer as O
    kfs, mps, cur = SC.toy_map(6)
    K, P = copy.deepcopy(kfs), copy.deepcopy(mps)
    gone = [m for m in P if cur in P[m]["obs"]][:20]
    for m in gone:
        del P[m]["obs"][cur]                                            # the tracking matched them; the key frame does not observe them yet
        if P[m]["ref_kf"] == cur:
            P[m]["ref_kf"] = min(P[m]["obs"])
    P[gone[0]]["bad"] = True
    done, recent = M.process_new_keyframe_points(H, cur, K, P)
    assert sorted(done) == sorted(gone[1:]) and all(cur in P[m]["obs"] for m in done) and set(recent) == {m for m in mps if cur in mps[m]["obs"]} - set(gone)
    assert all(P[m].get("normal") is not None and P[m].get("desc") is not None for m in done) and P[gone[0]].get("normal") is None
    done = M.update_after_fuse(H, cur, K, P)
    assert set(done) == {int(m) for m in K[cur]["mp"] if m >= 0 and not P[m].get("bad")}
    before = {m: P[m]["desc"].copy() for m in done}
    ids = sorted(P)[:30]
    for m in ids:
        P[m]["x3Dw"] = P[m]["x3Dw"] + np.float32(0.01)
    assert O.update_after_local_ba(H, K, P, dict(map_points=ids)) == [m for m in ids if not P[m].get("bad")]
    assert O.update_after_essential_graph(H, K, P, ids) == O.update_after_global_ba(H, K, P, dict(points={m: None for m in ids}))
    assert all(P[m]["desc"].tobytes() == before[m].tobytes() for m in before)      # the optimizers' step is UpdateNormalAndDepth alone
    one = M.map_points_item([ids[1]], K, P)
    ref = H.UpdateMapPoints([one])[0]
    assert P[ids[1]]["normal"].tobytes() == ref["normal"][0].tobytes() and np.float32(P[ids[1]]["max_dist"]).tobytes() == ref["max_dist"][0].tobytes()


def test_a_sanitizer_build_of_the_host_twins_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_triangulate, sindh_update_points and csrc/host/map_points.cpp with -fsanitize=address,undefined, run as a program of its own on the scenes of this file"""
    import mappoints_scene as SC
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mappoints_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "sindslam_amd", "csrc"), "sanitize-mappoints", "OUT=" + exe], check=True, capture_output=True, text=True)
    pairs = [(SC.tri_scene(50 + k, n, kind), 0) for k, (n, kind) in enumerate(((30, "mono"), (30, "stereo"), (65, "mixed"), (0, "mixed")))]
    pairs += [(p, 0) for p, _, _ in SC.tri_literal_cases().values()] + [(p, SIND_E_ARG) for p in SC.tri_bad_pairs().values()]
    items = [(SC.mp_scene(60, [1, 2, 3, 5, 0, 64, 65, 130]), 0), (SC.mp_scene(61, [4] * 30, flags=(True, False)), 0), (SC.mp_scene(62, [4] * 30, flags=(False, True)), 0), (SC.mp_scene(63, []), 0)]
    items += [(it, 0) for it, _ in SC.mp_literal_cases().values()] + [(it, SIND_E_ARG) for it in SC.mp_bad_items().values()]
    with open(tmp_path / "records.bin", "wb") as f:
        f.write(SC.K5.tobytes()); f.write(np.int32(len(SC.SCALE)).tobytes()); f.write(SC.SCALE.tobytes()); f.write(np.int32(len(pairs) + len(items)).tobytes())
        for p, rc in pairs:
            f.write(np.array([0, rc, len(p["kf1"]["octave"]), len(p["kf2"]["octave"])], np.int32).tobytes())
            for k in ("Tcw1", "Twc1", "Tcw2", "Twc2"):
                f.write(np.ascontiguousarray(p[k], np.float32).tobytes())
            for s in ("kf1", "kf2"):
                for k, t in (("xy", np.float32), ("un_xy", np.float32), ("octave", np.int32), ("u_right", np.float32), ("depth", np.float32)):
                    f.write(np.ascontiguousarray(p[s][k], t).tobytes())
            f.write(np.ascontiguousarray(p["match12"], np.int32).tobytes())
        for it, rc in items:
            f.write(np.array([1, rc, len(it["Ow"]), len(it["x3Dw"]), len(it["obs_kf"]), int(it["do_descriptor"]), int(it["do_normal"])], np.int32).tobytes())
            for k, t in (("Ow", np.float32), ("x3Dw", np.float32), ("obs_start", np.int32), ("obs_kf", np.int32), ("obs_bad", np.uint8), ("obs_octave", np.int32), ("obs_desc", np.uint8), ("ref_obs", np.int32)):
                f.write(np.ascontiguousarray(it[k], t).tobytes())
    r = subprocess.run([exe, str(tmp_path / "records.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(pairs) + len(items)
    H = SC.HostMap()
    for line, (p, rc) in zip(lines, pairs):                               # and it computed what the library computes
        got = [int(v) for v in line.split()]
        if rc:
            assert got[0] == rc
            continue
        g = H.Triangulate([p])[0]
        x = np.bitwise_xor.reduce(g["x3D"].view(np.uint32).ravel()) if g["x3D"].size else 0
        assert got == [0, g["nnew"], int(g["status"].sum()), int(x)], line
    for line, (it, rc) in zip(lines[len(pairs):], items):
        got = [int(v) for v in line.split()]
        if rc:
            assert got[0] == rc
            continue
        it = dict(it, desc=None, normal=None, max_dist=np.full(len(it["x3Dw"]), 7.0, np.float32), min_dist=None)
        g = H.UpdateMapPoints([it])[0]
        best = g["best_obs"] if it["do_descriptor"] else np.full(len(g["best_obs"]), 77)
        upd = g["updated"] if it["do_normal"] else np.full(len(g["updated"]), 7)
        x = np.bitwise_xor.reduce(g["max_dist"].view(np.uint32)) if g["max_dist"].size else 0
        assert got == [0, int(best.sum()), int(upd.astype(np.int64).sum()), int(x)], line
