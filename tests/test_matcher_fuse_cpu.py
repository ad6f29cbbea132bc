"""CPU: the Python restatement of the projections into a key frame (tests/fuse_ref.py: Fuse x 2, SearchByProjection(pKF, Scw), SearchBySim3) against properties
nothing else pins, the soundness of the caller's replay that include/sind_hip.h documents for sind_match_fuse, and the public surface of the new calls (C header,
Python methods) without a device."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def stream_scene(stream):
    import fuse_scene as FS
    return FS.stream_key_frame(stream, 7, seed=6)


@pytest.fixture(scope="module")
def stress_scene():
    import fuse_scene as FS
    return FS.stress_key_frame(1)


@pytest.fixture(scope="module")
def sim3_scene(stream):
    import fuse_ref as F
    import fuse_scene as FS
    args = FS.sim3_pair(stream, 6, seed=6)
    return args, F.search_by_sim3(*args, 7.5)


def test_public_header_declares_the_new_calls_as_c(tmp_path):
    src = tmp_path / "surface.c"
    src.write_text('#include "sind_hip.h"\n'
                   "int (*const fuse)(sind_match*, const sind_match_fuse_item*, int, float, int) = &sind_match_fuse;\n"
                   "int (*const by_projection_sim3)(sind_match*, const sind_match_proj_sim3*, int, int) = &sind_match_by_projection_sim3;\n"
                   "int (*const by_sim3)(sind_match*, const sind_match_sim3_pair*, int, float) = &sind_match_by_sim3;\n"
                   "int main(void) { return (int)(sizeof(sind_match_fuse_item) + sizeof(sind_match_proj_sim3) + sizeof(sind_match_sim3_pair) + sizeof(sind_match_sim3_side)); }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_matcher_has_the_new_methods():
    from sindslam_amd.matcher import ORBmatcher                             # importing the module loads no library
    assert all(callable(getattr(ORBmatcher, k)) for k in ("Fuse", "FuseSim3", "SearchByProjectionSim3", "SearchBySim3"))


def _check_point_match(F, mode, cam, sc, T, Ow, mp, kf, th, i, k, limit, T2=None):
    """point i matched keypoint k: inside the window of its projection, in its level range, at or below the threshold"""
    why, u, v, invz, lv = F.project(mode, cam, sc, T, Ow, mp["x3Dw"][i], None if mode == F.BY_SIM3 else mp["normal"][i], mp["max_dist"][i], mp["min_dist"][i], T2=T2)
    assert why == F.IN_VIEW and mp["valid"][i]
    rad = f32(f32(th) * sc[lv])
    assert abs(f32(kf["un_xy"][k, 0] - u)) < rad and abs(f32(kf["un_xy"][k, 1] - v)) < rad
    assert lv - 1 <= kf["octave"][k] <= lv
    assert F.hamming(mp["desc"][i], kf["desc"][k]) <= limit
    return u, v, invz


def test_every_match_is_inside_its_window_level_range_and_threshold(stream_scene, stress_scene, sim3_scene):
    import fuse_ref as F
    import fuse_scene as FS
    import localmap_ref as R
    total = 0
    for cam, sc, Tc, mp, kf in (stream_scene, stress_scene):
        for sim3, th in ((0, 3.0), (1, 4.0)):
            T = FS.similarity(Tc, 0.93) if sim3 else Tc
            o = F.fuse_search(cam, sc, T, mp, kf, th, sim3)
            Tm, Ow = F._pose(T, sim3)
            hit = np.nonzero(o["best_idx"] >= 0)[0]
            assert len(hit) == o["nfused"] and (o["best_dist"][o["best_idx"] < 0] == -1).all()
            for i in hit[::5]:
                u, v, invz = _check_point_match(F, F.FUSE_SIM3 if sim3 else F.FUSE, cam, sc, Tm, Ow, mp, kf, th, i, o["best_idx"][i], F.TH_LOW)
                assert o["best_dist"][i] == F.hamming(mp["desc"][i], kf["desc"][o["best_idx"][i]])
                if not sim3: assert F.chi2_ok(cam, sc, kf, o["best_idx"][i], u, v, invz)[0]
            total += len(hit)
        S = FS.similarity(Tc, 1.08); Tm, Ow = F._pose(S, True)
        m, nm, choice, _ = F.search_kf_sim3(cam, sc, S, mp, kf, 10)
        assert (m >= 0).sum() == nm == (choice >= 0).sum()                    # every match closes its keypoint: nothing is overwritten
        assert (m[kf["taken"] > 0] == -1).all()
        for k in np.nonzero(m >= 0)[0][::5]:
            _check_point_match(F, F.PROJ_SIM3, cam, sc, Tm, Ow, mp, kf, 10, m[k], k, F.TH_LOW)
        total += nm
    (cam, sc, T1w, T2w, s12, R12, t12, s1, s2), (m12, nf, vn1, vn2, _, _) = sim3_scene
    T21, T12 = F.sim3_transforms(s12, R12, t12)
    for src, dst, vn, Tw, T2 in ((s1, s2, vn1, T1w, T21), (s2, s1, vn2, T2w, T12)):
        pts = dict(src, desc=src["mp_desc"]); keys = dict(dst, desc=dst["kf_desc"])
        for i in np.nonzero(vn >= 0)[0][::5]:
            _check_point_match(F, F.BY_SIM3, cam, sc, np.asarray(Tw, f32), None, pts, keys, 7.5, i, vn[i], F.TH_HIGH, T2=T2)
    assert total > 4000                                                      # found: 9068 matches over the two scenes and three searches


def test_key_frame_window_walk_equals_brute_force_over_all_keypoints(stream_scene, stress_scene):
    import fuse_ref as F
    for cam, sc, Tc, mp, kf in (stream_scene, stress_scene):
        o = F.fuse_search(cam, sc, Tc, mp, kf, 3.0, 0)
        total = 0
        for th in (3.0, 10.0):
            for i in np.nonzero(o["why"] == F.IN_VIEW)[0][::7]:
                x, y = o["proj"][i]; rad = f32(f32(th) * sc[o["level"][i]])
                got = F.kf_features_in_area(cam, kf, x, y, rad)
                dx = np.abs((kf["un_xy"][:, 0] - x).astype(f32)); dy = np.abs((kf["un_xy"][:, 1] - y).astype(f32))
                assert len(got) == len(set(got)) and sorted(got) == np.nonzero((dx < rad) & (dy < rad))[0].tolist()     # no level argument: every octave
                total += len(got)
        assert total > 1000


def test_key_frame_bounds_are_the_frames_truncated_and_the_cell_size_is_not():
    import fuse_ref as F
    cam = np.array([500, 500, 320, 240, 40, 0.08, -12.7, 655.4, -9.2, 489.9], f32)
    kb, w_inv, h_inv = F.kf_bounds(cam)
    assert kb == [f32(-12), f32(655), f32(-9), f32(489)]
    assert w_inv == f32(f32(64) / f32(f32(655.4) - f32(-12.7))) and h_inv == f32(f32(48) / f32(f32(489.9) - f32(-9.2)))


def test_each_branch_scene_point_leaves_by_the_exit_it_was_built_for():
    import fuse_ref as F
    import fuse_scene as FS
    import localmap_ref as R
    cam, sc, Tc, mp, kf, expect = FS.branch_scene()
    frustum = R.frustum(cam, sc, Tc, dict(mp, flags=mp["valid"] * 3))
    m_proj = F.search_kf_sim3(cam, sc, FS.similarity(Tc, 1.08), mp, kf, 10)
    for sim3 in (0, 1):
        o = F.fuse_search(cam, sc, FS.similarity(Tc, 0.93) if sim3 else Tc, mp, kf, 4.0 if sim3 else 3.0, sim3)
        seen = set()
        for i, (why, lvl, name) in enumerate(expect):
            assert o["why"][i] == why and m_proj[3][i] == why, (i, name, sim3)
            if name == "at_max_x":
                assert frustum["in_view"][i] and o["proj"][i, 0] == 0             # in for isInFrustum (u <= mnMaxX), out here (u < mnMaxX)
            if why == F.IN_VIEW and lvl is not None and not sim3:
                assert o["level"][i] == lvl, (i, name)
            seen.add(name)
        assert {e[0] for e in expect} == {F.IN_VIEW, F.BEHIND, F.OUT_X, F.OUT_Y, F.OUT_DIST, F.OUT_ANGLE, F.NOT_CANDIDATE}
        assert seen >= {"behind", "left", "right", "above", "below", "at_max_x", "too_near", "too_far", "oblique", "not_candidate", "level_0", "level_top"} | {f"created_{k}" for k in range(len(sc))}


def test_chi_square_rejects_and_passes_stereo_and_mono_candidates(stream_scene):
    import fuse_ref as F
    cam, sc, Tc, mp, kf = stream_scene
    st = F.fuse_search(cam, sc, Tc, mp, kf, 3.0, 0)["stats"]
    assert min(st.values()) > 50, st                                         # found: stereo 1954 pass / 467 reject, mono 669 pass / 122 reject
    assert (kf["u_right"] < 0).sum() > 200 and (kf["u_right"] >= 0).sum() > 200


def test_search_by_sim3_agreement_and_prematched_slots(sim3_scene):
    (cam, sc, T1w, T2w, s12, R12, t12, s1, s2), (m12, nf, vn1, vn2, why1, why2) = sim3_scene
    assert s12 != 1 and (s1["valid"] == 0).sum() > 100 and (s2["valid"] == 0).sum() > 100
    agree = np.array([v >= 0 and vn2[v] == i for i, v in enumerate(vn1)])
    assert nf == agree.sum() == (m12 >= 0).sum() > 200 and ((vn1 >= 0) & ~agree).sum() > 100      # found: 427 agreeing, 342 one-way only
    assert np.array_equal(m12[agree], vn1[agree]) and (m12[~agree] == -1).all()
    assert (vn1[s1["valid"] == 0] == -1).all() and (vn2[s2["valid"] == 0] == -1).all()             # no pre-matched slot is rematched
    assert (m12[s1["valid"] == 0] == -1).all() and s2["valid"][m12[m12 >= 0]].all()


def test_search_by_projection_sim3_depends_on_the_order_of_the_points(stream_scene, stress_scene):
    import fuse_ref as F
    import fuse_scene as FS
    for cam, sc, Tc, mp, kf in (stream_scene, stress_scene):
        S = FS.similarity(Tc, 1.08)
        m, nm, choice, _ = F.search_kf_sim3(cam, sc, S, mp, kf, 10)
        _, nm0, choice0, _ = F.search_kf_sim3(cam, sc, S, mp, kf, 10, sequential=False)
        assert (choice != choice0).sum() > 100 and nm0 > nm, "the scene is wrong"     # found on the stream scene: 893 choices differ, 747 matches against 1609
        first = {}
        for i, k in enumerate(choice0):
            if k >= 0: first.setdefault(int(k), i)
        assert all(choice[i] == k for k, i in first.items() if not any(choice[j] == k for j in range(i)))


# ---- the caller's replay of the tail of Fuse on a toy graph ----
@pytest.mark.parametrize("sim3", [0, 1])
@pytest.mark.parametrize("seed", [1, 2])
def test_replay_after_the_snapshot_search_leaves_the_graph_of_the_sequential_loop(seed, sim3):
    import fuse_ref as F
    import fuse_scene as FS
    g, cam, sc, Tc, kf, plist, n_list = FS.toy_graph(seed)
    T = FS.similarity(Tc, 0.93) if sim3 else Tc
    th = 4.0 if sim3 else 3.0
    full = F.clone(g); n_full, rp_full = F.fuse_full(full, cam, sc, T, 0, kf, plist, th, sim3)
    snap = F.fuse_search(cam, sc, T, g.inputs(0, plist, sim3), kf, th, sim3)
    rep = F.clone(g); n_rep, rp_rep = F.fuse_replay(rep, snap["best_idx"], 0, plist, sim3)
    assert n_rep == n_full > 190 and rp_rep == rp_full and rep.state() == full.state() and rep.log == full.log      # found: 388 / 387 (Fuse), 417 / 420 (Scw) of 445 entries
    assert full.state() != g.state()
    kinds = [e[0] for e in full.log]
    assert kinds.count("add") > 37 and kinds.count("bad_in_kf") > 28          # free keypoints, and keypoints occupied by a bad point; found: 74 / 82 and 66 / 56 (248 Replace calls)
    added = {}
    for e in full.log:
        if e[0] == "add": added[e[1]] = e[2]
    if sim3:
        assert sum(p >= 0 for p in rp_full) > 10
        assert any(p >= 0 and p < n_list and p != plist[i] for i, p in enumerate(rp_full))       # several points on one keypoint: the first is added, the second gets it as vpReplacePoint
        assert any(p >= 0 and p == plist[i] for i, p in enumerate(rp_full))                      # a repeated entry finds itself
        assert n_rep == snap["nfused"]
    else:
        rep_log = [e for e in full.log if e[0] == "replace"]
        assert any(l < n_list and s >= n_list for _, l, s in rep_log) and any(l >= n_list and s < n_list for _, l, s in rep_log)      # resident wins / resident loses: both Observations() orders
        assert any(l < n_list and s in added for _, l, s in rep_log) and any(l in added and s < n_list for _, l, s in rep_log)        # add, then replace, in both orders
        seen, caught = set(), 0
        for i, pid in enumerate(plist):
            if pid >= 0 and pid in seen and snap["best_idx"][i] >= 0: caught += 1
            seen.add(pid)
        assert caught > 0 and n_rep < snap["nfused"]                          # repeated entries the snapshot search matched again: the re-test skips them


def test_batching_two_key_frames_from_one_snapshot_is_not_the_sequential_run():
    """the documented caveat: key frame 0's Replace calls change the list for key frame 1 (bad flags are caught by the re-test, recomputed descriptors are not)"""
    import fuse_ref as F
    import fuse_scene as FS
    g, cam, sc, Tc, kf, plist, _ = FS.toy_graph(1)
    seq = F.clone(g)
    n_seq = [F.fuse_full(seq, cam, sc, Tc, k, kf, plist, 3.0, 0)[0] for k in (0, 1)]
    bat = F.clone(g)
    snaps = [F.fuse_search(cam, sc, Tc, g.inputs(k, plist, 0), kf, 3.0, 0)["best_idx"] for k in (0, 1)]
    n_bat = [F.fuse_replay(bat, snaps[k], k, plist, 0)[0] for k in (0, 1)]
    assert n_bat[0] == n_seq[0]
    assert n_bat[1] != n_seq[1] and bat.state() != seq.state()
    one = F.clone(g)                                                          # one item per call with refreshed inputs is exact
    n_one = [F.fuse_replay(one, F.fuse_search(cam, sc, Tc, one.inputs(k, plist, 0), kf, 3.0, 0)["best_idx"], k, plist, 0)[0] for k in (0, 1)]
    assert n_one == n_seq and one.state() == seq.state()
