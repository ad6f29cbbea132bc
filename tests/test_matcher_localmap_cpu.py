"""CPU: the Python restatement of the map-point projection searches (tests/localmap_ref.py) against properties nothing else pins, and the
public surface of the new calls (C header, Python methods) without a device."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def stream_scene(stream):
    import localmap_ref as R
    import localmap_scene as L
    cam, sc, Tc, mp, cur = L.stream_local_map(stream, 6, seed=6)
    return cam, sc, Tc, mp, cur, R.frustum(cam, sc, Tc, mp)


@pytest.fixture(scope="module")
def stress_scene():
    import localmap_ref as R
    import localmap_scene as L
    cam, sc, Tc, mp, cur = L.stress_local_map(1)
    return cam, sc, Tc, mp, cur, R.frustum(cam, sc, Tc, mp)


def _check_matches(cam, sc, mp, cur, fr, th, m):
    import localmap_ref as R
    n = 0
    for k in np.nonzero(m >= 0)[0]:
        i = m[k]; lv = fr["level"][i]; x, y, xr = fr["proj_xyr"][i]
        rad = R.local_radius(fr["view_cos"][i], th, sc, lv)
        assert fr["in_view"][i] and (mp["flags"][i] & 1)
        assert abs(f32(cur["un_xy"][k, 0] - x)) < rad and abs(f32(cur["un_xy"][k, 1] - y)) < rad
        assert lv - 1 <= cur["octave"][k] <= lv
        assert R.hamming(mp["desc"][i], cur["desc"][k]) <= R.TH_HIGH
        assert not (cur["u_right"][k] > 0 and abs(f32(xr - cur["u_right"][k])) > rad)
        n += 1
    return n


@pytest.mark.parametrize("th", [1, 3, 5])
def test_every_match_is_inside_its_window_level_range_and_threshold(stream_scene, stress_scene, th):
    import localmap_ref as R
    for cam, sc, Tc, mp, cur, fr in (stream_scene, stress_scene):
        m, nm, choice, _ = R.search_local(cam, sc, mp, cur, fr, th)
        assert _check_matches(cam, sc, mp, cur, fr, th, m) == (m >= 0).sum() <= nm
        assert (choice >= 0).sum() == nm                                      # nmatches counts every assignment, overwritten ones included


def test_stream_scene_has_both_radius_classes_and_the_viewing_angle_exit(stream_scene):
    import localmap_ref as R
    cam, sc, Tc, mp, cur, fr = stream_scene
    iv = fr["in_view"] > 0
    narrow = (fr["view_cos"][iv].astype(f64) > 0.998).sum()
    assert narrow > 1000 and iv.sum() - narrow > 100 and (fr["why"] == R.OUT_ANGLE).sum() > 100 and (fr["why"] == R.NOT_CANDIDATE).sum() > 100
    assert fr["n_to_match"] == iv.sum()


def test_no_taken_keypoint_is_reassigned_and_observed_points_close_theirs(stress_scene):
    import localmap_ref as R
    cam, sc, Tc, mp, cur, fr = stress_scene
    m, nm, choice, _ = R.search_local(cam, sc, mp, cur, fr, 5)
    assert cur["taken"].sum() > 100 and (m[cur["taken"] > 0] == -1).all()
    overwritten = 0
    for i in np.nonzero(choice >= 0)[0]:
        later = np.nonzero(choice[i + 1:] == choice[i])[0]
        if mp["flags"][i] & 2:
            assert len(later) == 0                                            # a point with observations closes its keypoint
        else:
            overwritten += len(later) > 0
    assert overwritten > 0 and nm - (m >= 0).sum() == overwritten           # found here: 1004 assignments at th 5


def test_with_all_points_observed_nmatches_counts_the_assigned_keypoints(stress_scene):
    import localmap_ref as R
    cam, sc, Tc, mp, cur, fr = stress_scene
    mp = dict(mp); mp["flags"] = mp["flags"] | 2
    m, nm, _, _ = R.search_local(cam, sc, mp, cur, fr, 5)
    assert nm == (m >= 0).sum() > 400


def test_window_search_equals_brute_force_over_all_keypoints(stream_scene, stress_scene):
    import localmap_ref as R
    for cam, sc, Tc, mp, cur, fr in (stream_scene, stress_scene):
        idx = np.nonzero(fr["in_view"])[0][::7]
        total = 0
        for th in (1, 3, 5):
            for i in idx:
                lv = int(fr["level"][i]); x, y, _ = fr["proj_xyr"][i]
                rad = R.local_radius(fr["view_cos"][i], th, sc, lv)
                got = R.features_in_area(cam, cur, x, y, rad, lv - 1, lv)
                dx = np.abs((cur["un_xy"][:, 0] - x).astype(f32)); dy = np.abs((cur["un_xy"][:, 1] - y).astype(f32))
                want = np.nonzero((dx < rad) & (dy < rad) & (cur["octave"] >= lv - 1) & (cur["octave"] <= lv))[0]
                assert len(got) == len(set(got)) and sorted(got) == want.tolist()
                total += len(got)
        assert total > 1000


def test_each_branch_scene_point_leaves_by_the_exit_it_was_built_for():
    import localmap_ref as R
    import localmap_scene as L
    cam, sc, Tc, mp, cur, expect = L.branch_scene()
    fr = R.frustum(cam, sc, Tc, mp)
    Ow = R.camera_centre(Tc)
    seen = set()
    for i, (why, rc, lvl, name) in enumerate(expect):
        assert fr["why"][i] == why, (i, name)
        assert fr["in_view"][i] == (why == R.IN_VIEW)
        if why != R.IN_VIEW:
            assert fr["level"][i] == 0 and fr["view_cos"][i] == 0 and (fr["proj_xyr"][i] == 0).all()
            continue
        assert (R.radius_by_viewing_cos(fr["view_cos"][i]) == f32(2.5)) == (rc == "narrow"), (i, name)
        if lvl is not None:
            assert fr["level"][i] == lvl, (i, name)
        if name.startswith("created_"):
            assert f32(mp["max_dist"][i] / R.distance(mp["x3Dw"][i], Ow)[1]) == sc[lvl]       # the case the definition of log decides
        seen.add(name)
    assert {e[0] for e in expect} == {R.IN_VIEW, R.BEHIND, R.OUT_X, R.OUT_Y, R.OUT_DIST, R.OUT_ANGLE, R.NOT_CANDIDATE}
    assert seen >= {"narrow", "wide", "level_0", "level_top"} | {f"created_{o}" for o in range(len(sc))}
    assert fr["n_to_match"] == sum(e[0] == R.IN_VIEW for e in expect)


def test_th_one_leaves_the_radius_unscaled():
    import localmap_ref as R
    import match_scene as S
    sc = S._scale_factors()
    for vc, r in ((f32(0.9981), f32(2.5)), (f32(0.998), f32(2.5)), (f32(0.9979), f32(4.0)), (f32(0.5), f32(4.0))):    # (double)0.998f > 0.998: against the double literal the float nearest to 0.998 is narrow
        for lv in range(8):
            assert R.local_radius(vc, 1, sc, lv) == f32(r * sc[lv])
            assert R.local_radius(vc, 3, sc, lv) == f32(f32(r * f32(3)) * sc[lv])


def test_public_header_declares_the_new_calls_as_c(tmp_path):
    src = tmp_path / "surface.c"
    src.write_text('#include "sind_hip.h"\n'
                   "int (*const reserve)(sind_match*, int) = &sind_match_reserve_map_points;\n"
                   "int (*const local_map)(sind_match*, const sind_match_local*, int, float, float, float) = &sind_match_local_map;\n"
                   "int (*const by_projection_kf)(sind_match*, const sind_match_reloc*, int, float, int, int) = &sind_match_by_projection_kf;\n"
                   "int main(void) { return (int)(sizeof(sind_match_local) + sizeof(sind_match_reloc)); }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_matcher_has_the_new_methods():
    from sindslam_amd.matcher import ORBmatcher                             # importing the module loads no library
    assert callable(ORBmatcher.SearchLocalPoints) and callable(ORBmatcher.SearchByProjectionKF) and callable(ORBmatcher.reserve_map_points)
