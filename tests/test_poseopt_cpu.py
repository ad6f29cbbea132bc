"""CPU: the host twin of sind_match_pose_optimize (sindh_pose_optimize; csrc/host/pose_opt.hpp, csrc/host/pose_opt.cpp) against the Python restatement
tests/poseopt_ref.py, bit for bit; the literal semantics of Optimizer::PoseOptimization (reference src/Optimizer.cc:239-451), each on its own small scene; planted
outliers; scipy's least squares, which shares nothing with the code under test; the defined sin / cos; and the relocalisation chain (sindslam_amd/optimizer.py)."""
import ctypes as C

import numpy as np
import pytest


def _ref(s, trace=None):
    import poseopt_ref as R
    import poseopt_scene as P
    return R.pose_optimization(s["x3Dw"], s["obs_xy"], s["u_right"], s["inv_sigma2"], s["Tcw"], P.K5, trace)


def _host(s):
    import poseopt_scene as P
    return P.HostOptimizer().PoseOptimization([s])[0]


@pytest.fixture(scope="module")
def traced():
    """the n = 65 mixed scene: the host's result, the restatement's, and the restatement's trace"""
    import poseopt_scene as P
    s = P.scene(65, 65, "mixed")
    tr = []
    return s, _host(s), _ref(s, tr), tr


@pytest.mark.parametrize("n", [3, 9, 10, 65])
def test_host_library_equals_the_restatement_bit_for_bit(n, traced):
    import poseopt_scene as P
    if n == 65:
        P.assert_same(traced[1], traced[2], n)
    for kind in ("mixed", "mono", "stereo") if n != 65 else ("stereo",):
        s = P.scene(n + {"mixed": 0, "mono": 100, "stereo": 200}[kind], n, kind)
        P.assert_same(_host(s), _ref(s), (n, kind))


def test_two_correspondences_return_zero_and_leave_the_pose():
    import poseopt_scene as P
    from sindslam_amd.matcher import poseopt_items
    s = P.scene(2, 2, "mixed", outliers=0)
    arr, keep = poseopt_items([s])
    a = keep[0]
    a["Tcw_out"][:] = 7.0; a["outlier"][:] = 9; a["n_good"][:] = -5; a["n_rounds"][:] = -5; a["round_iters"][:] = 3
    assert P.host().sindh_pose_optimize(arr, 1, *P.HostOptimizer().K) == 0
    assert a["n_good"][0] == 0 and a["n_rounds"][0] == 0
    assert (a["Tcw_out"] == 7.0).all() and (a["outlier"] == 9).all() and (a["round_iters"] == 3).all()      # `return 0` comes before SetPose
    r = _ref(s)
    assert r["n_good"] == 0 and r["n_rounds"] == 0 and r["Tcw"] is None


def test_nine_correspondences_run_one_round_only():
    import poseopt_scene as P
    g = _host(P.scene(9, 9, "mixed"))
    assert g["n_rounds"] == 1 and g["round_iters"][0] > 0 and (g["round_iters"][1:] == 0).all()
    assert g["n_good"] == 9 - g["round_nbad"][0]
    assert _host(P.scene(10, 10, "mixed"))["n_rounds"] == 4              # edges().size() < 10 is the only way out


def test_every_round_restarts_from_the_input_pose(traced):
    """round 1's first linearisation has the chi2 of the INPUT pose over the edges round 0 left at level 0, not that of round 0's result"""
    import poseopt_ref as R
    import poseopt_scene as P
    s, g, r, tr = traced
    K = [np.float64(np.float32(k)) for k in P.K5]
    n = len(s["u_right"])
    edges = [([np.float64(v) for v in s["x3Dw"][i]], np.float64(s["obs_xy"][i, 0]), np.float64(s["obs_xy"][i, 1]), np.float64(s["u_right"][i]), np.float64(s["inv_sigma2"][i]),
              not bool(s["u_right"][i] < 0)) for i in range(n)]
    for rnd in (1, 2, 3):
        level = [t for t in tr if t[0] == rnd - 1 and t[1] == "classified"][0][2]
        ini = [t for t in tr if t[0] == rnd and t[1] == 0 and len(t) == 3][0][2]
        with np.errstate(all="ignore"):
            at_input = R.sums(R.from_tcw(s["Tcw"]), K, edges, level, rnd < 3, False)[27]
            q = r["round_pose"][rnd - 1]
            prev = R.se3([[np.float64(q[3 * a + c]) for c in range(3)] for a in range(3)], [np.float64(v) for v in q[9:]])
            at_prev = R.sums(prev, K, edges, level, rnd < 3, False)[27]
        assert P.bits(np.float64(ini)) == P.bits(np.float64(at_input)), rnd
        assert ini > 2 * at_prev                                         # the two are far apart on this scene, so the equality above decides


def test_an_edge_flagged_in_round_0_returns_as_an_inlier_in_round_3():
    import poseopt_scene as P
    s = P.scene(10, 10, "mixed")
    tr = []
    r = _ref(s, tr)
    g = _host(s)
    P.assert_same(g, r, "scene")
    first = np.array([t for t in tr if t[0] == 0 and t[1] == "classified"][0][2])
    back = first & ~g["outlier"].astype(bool)
    assert back.any() and g["round_nbad"][0] > g["round_nbad"][3]
    assert not s["is_outlier"][back].any()                               # and they are true inliers that the bad start had pushed out


def test_a_point_at_depth_zero_is_counted_as_the_float_compare_counts_it():
    """z = 0 under the input pose: the stereo edge's chi2 is NaN (inf - inf), H and every trial's chi2 are NaN; a NaN tempChi rejects every step, so the pose stays; and
    `chi2 > 7.815f` is false for a NaN, so the edge, and every edge judged at a NaN trial pose, counts as an inlier"""
    import poseopt_scene as P
    s = P.behind_camera()
    tr = []
    r = _ref(s, tr)
    g = _host(s)
    P.assert_same(g, r, "z = 0")
    trials = [t for t in tr if len(t) == 5]
    assert trials and all(np.isnan(t[3]) and not t[4] for t in trials)
    for t in (t for t in tr if t[1] == "classified"):
        chi2 = np.array(t[3]); thr = np.where(s["u_right"] < 0, np.float32(5.991), np.float32(7.815))
        assert not np.isfinite(chi2[4])
        with np.errstate(invalid="ignore"):
            assert np.array_equal(np.array(t[2]), chi2 > thr)
    assert g["n_rounds"] == 4 and g["n_good"] == len(s["u_right"]) - int(g["outlier"].sum())
    assert np.isfinite(g["Tcw"]).all() and np.abs(g["Tcw"] - s["Tcw"]).max() < 1e-6


def test_identical_points_make_a_rank_deficient_system_and_the_call_returns():
    import poseopt_scene as P
    s = P.identical_points()
    tr = []
    r = _ref(s, tr)
    g = _host(s)
    P.assert_same(g, r, "identical")
    assert g["n_rounds"] == 4 and (g["round_iters"] < 10).all() and (g["round_iters"] > 0).all()      # Terminate on a rejected step (rho == 0), well before ten
    last = [t for t in tr if len(t) == 5 and t[0] == 0][-1]
    assert not last[4]
    assert np.isfinite(g["Tcw"]).all() and np.isfinite(g["round_pose"]).all()


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_planted_outliers_are_exactly_the_flags(kind):
    import poseopt_scene as P
    n = 80
    s = P.scene(7, n, kind, outliers=int(0.3 * n), noise=0.0)
    g = _host(s)
    assert np.array_equal(g["outlier"].astype(bool), s["is_outlier"])
    assert g["n_good"] == n - int(0.3 * n)


def _scipy_pose(s, keep, start):
    """plain weighted least squares over the kept edges with scipy, from the pose `start` [R | t]: -> [R row-major | t]"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    import poseopt_scene as P
    fx, fy, cx, cy, bf = (float(np.float32(k)) for k in P.K5)
    X = s["x3Dw"][keep].astype(np.float64); o = s["obs_xy"][keep].astype(np.float64); ur = s["u_right"][keep].astype(np.float64)
    w = np.sqrt(s["inv_sigma2"][keep].astype(np.float64)); st = ur >= 0
    R0, t0 = np.asarray(start[:9]).reshape(3, 3), np.asarray(start[9:])

    def pose(u):
        dR = Rotation.from_rotvec(u[:3]).as_matrix()
        return dR @ R0, dR @ t0 + u[3:]

    def res(u):
        R, t = pose(u)
        Xc = X @ R.T + t
        px = fx * Xc[:, 0] / Xc[:, 2] + cx; py = fy * Xc[:, 1] / Xc[:, 2] + cy
        return np.concatenate([w * (o[:, 0] - px), w * (o[:, 1] - py), (w * (ur - (px - bf / Xc[:, 2])))[st]])

    sol = least_squares(res, np.zeros(6), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    R, t = pose(sol.x)
    return np.concatenate([R.reshape(-1), t])


def test_round_3_is_the_weighted_least_squares_minimum_scipy_finds(traced):
    """Round 3 has no robust kernel and its inlier set is fixed (round 2's classification), so its pose is a plain weighted least-squares minimiser up to where g2o's
    ten iterations stop.  Floor = the distance between two scipy minimisers from different starts (the input pose, round 3's pose); allowed: ten times that.
    Measured on this scene (max over the 12 entries of [R | t]): see profiles/match_pose_opt.txt."""
    pytest.importorskip("scipy")
    s, g, r, tr = traced
    keep = ~np.array([t for t in tr if t[0] == 2 and t[1] == "classified"][0][2])
    T = s["Tcw"].astype(np.float64)
    a = _scipy_pose(s, keep, np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]))
    b = _scipy_pose(s, keep, g["round_pose"][3])
    floor = np.abs(a - b).max()
    dist = np.abs(g["round_pose"][3] - a).max()
    print(f"scipy floor {floor:.3e}, product to scipy {dist:.3e}")
    assert dist <= 10 * floor, (dist, floor)


def test_defined_sincos_against_numpy():
    import poseopt_ref as R
    import poseopt_scene as P
    x = np.concatenate([np.linspace(1e-5, np.pi, 100000), [4.0, 7.5, 10.0, 100.0, 1234.5678, 1e4, 98765.4321, 1e5, -2.5, -1e3]])
    sn = np.zeros_like(x); cs = np.zeros_like(x)
    P.host().sindh_poseopt_sincos(C.c_void_p(x.ctypes.data), len(x), C.c_void_p(sn.ctypes.data), C.c_void_p(cs.ctypes.data))
    ulps = lambda a, b: int(np.abs(a.view(np.int64) - b.view(np.int64)).max())
    assert ulps(sn, np.sin(x)) <= 1 and ulps(cs, np.cos(x)) <= 1
    z = np.array([0.0, np.nan]); sn = np.ones(2); cs = np.zeros(2)
    P.host().sindh_poseopt_sincos(C.c_void_p(z.ctypes.data), 2, C.c_void_p(sn.ctypes.data), C.c_void_p(cs.ctypes.data))
    assert sn[0] == 0.0 and not np.signbit(sn[0]) and cs[0] == 1.0 and np.isnan(sn[1]) and np.isnan(cs[1])
    for v in (0.0, 1e-5, 0.3, 2.0, 1234.5678):                            # the restatement's is the same function
        k = int(np.argmin(np.abs(x - v))) if v else None
        got = R.sincos(np.float64(x[k] if v else 0.0))
        ref = (sn[0], cs[0]) if not v else None
        if v:
            a = np.zeros(1); b = np.zeros(1); w = np.array([x[k]])
            P.host().sindh_poseopt_sincos(C.c_void_p(w.ctypes.data), 1, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data)); ref = (a[0], b[0])
        assert P.bits(np.float64(got[0])) == P.bits(np.float64(ref[0])) and P.bits(np.float64(got[1])) == P.bits(np.float64(ref[1]))


# ---------------------------------------------------------------- the relocalisation chain on a toy with scripted searches
def _toy(n_pnp, add1=(0, 0), add2=(0, 0), N=140):
    """A frame of N keypoints that all have a true map point; the candidate matched the first n_pnp of them (all PnP inliers).  The first scripted search adds add1[0] good
    keypoints and add1[1] whose observation is grossly wrong, the second add2 likewise.  -> frame, candidates, search"""
    import poseopt_scene as P
    s = P.scene(77, N, "mixed", outliers=0, noise=0.0)
    frame = dict(un_xy=s["obs_xy"].copy(), u_right=s["u_right"].copy(), inv_sigma2=s["inv_sigma2"], mp=np.full(N, -1, np.int64), x3Dw=np.zeros((N, 3), np.float32), Tcw=s["Tcw"])
    cand = dict(match_mp=np.where(np.arange(N) < n_pnp, 1000 + np.arange(N), -1), match_x3Dw=s["x3Dw"])
    at = [n_pnp]; script = []
    for good, bad in (add1, add2):
        j = np.arange(at[0], at[0] + good + bad); at[0] += good + bad
        for k in j[good:]:
            frame["un_xy"][k] += 60.0
        script.append(j)
    calls = []

    def search(i, f, sFound, th, ORBdist):
        j = script[len(calls)]; calls.append((th, ORBdist, sorted(sFound)))
        assert not (f["mp"][j] >= 0).any() and not set(1000 + j) & set(sFound)
        f["mp"][j] = 1000 + j; f["x3Dw"][j] = s["x3Dw"][j]
        return len(j)
    return frame, [cand], search, calls, s


@pytest.mark.parametrize("case", ["continue", "direct", "search1_short", "optimize2_enough", "optimize2_low", "search2_short", "optimize3"])
def test_relocalization_accept_takes_every_branch(case):
    import poseopt_scene as P
    from sindslam_amd.optimizer import relocalization_accept
    n_pnp, add1, add2, steps, verdict = {
        "continue": (8, (0, 0), (0, 0), ["optimize1", "continue"], False),                                # :1479
        "direct": (60, (0, 0), (0, 0), ["optimize1", "verdict"], True),                                     # nGood >= 50 at once
        "search1_short": (20, (10, 0), (0, 0), ["optimize1", "search1", "verdict"], False),                 # :1491 fails
        "optimize2_enough": (20, (40, 0), (0, 0), ["optimize1", "search1", "optimize2", "verdict"], True),  # :1493, then neither :1497
        "optimize2_low": (20, (5, 25), (0, 0), ["optimize1", "search1", "optimize2", "verdict"], False),    # nGood 25 <= 30
        "search2_short": (20, (15, 15), (5, 0), ["optimize1", "search1", "optimize2", "search2", "verdict"], False),   # :1506 fails
        "optimize3": (20, (15, 15), (20, 0), ["optimize1", "search1", "optimize2", "search2", "optimize3", "verdict"], True),
    }[case]
    frame, cands, search, calls, s = _toy(n_pnp, add1, add2)
    trace = []
    accept = relocalization_accept(P.HostOptimizer(), frame, cands, search=search, trace=trace)
    vb = np.arange(len(frame["mp"])) < n_pnp
    assert accept(0, s["Tcw"], vb, n_pnp) is verdict
    assert [t[0] for t in trace] == steps, trace
    got = dict((t[0], t[1] if len(t) > 1 else None) for t in trace)
    assert got["optimize1"] == n_pnp
    if "optimize2" in got:
        assert got["optimize2"] == n_pnp + add1[0]
        assert calls[0][:2] == (10, 100) and calls[0][2] == list(range(1000, 1000 + n_pnp))
    if "search2" in got:                                                # sFound = every keypoint that still holds a point: the second optimisation's outliers too
        assert calls[1][:2] == (3, 64) and calls[1][2] == list(range(1000, 1000 + n_pnp + sum(add1)))
    if "optimize3" in got:
        assert got["optimize3"] == n_pnp + add1[0] + add2[0]
        assert int((frame["mp"] >= 0).sum()) == got["optimize3"]        # :1510-1512 cleared the outliers' matches
    elif "optimize2" in got:
        assert int((frame["mp"] >= 0).sum()) == n_pnp + sum(add1) + sum(add2[:1] if "search2" in got else ())      # :1493 does not clear them
