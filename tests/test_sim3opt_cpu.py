"""CPU: the host twin of sind_match_sim3_optimize (sindh_sim3_optimize; csrc/host/sim3_opt.hpp, csrc/host/sim3_opt.cpp) against the Python restatement
tests/sim3opt_ref.py, bit for bit; the defined exp; the numeric Jacobian against the analytic one; recovery of a known Sim3 and scipy's minimum of the same Huber
cost, which shares nothing with the code under test; planted outliers; the early returns; the degenerate scenes; a stand-alone sanitizer build; and the Python
layer of sindslam_amd/optimizer.py on toys.  The measured figures named below are in profiles/match_sim3_opt.txt."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

EXP_ULPS = 1                                                            # measured: the largest distance of the defined exp from math.exp over the sweep below
JACOBIAN_DEVIATION = 9.81e-8                                               # measured: numeric against analytic, relative to the largest entry of the edge's Jacobian
RECOVERY = 1.10e-7                                                        # measured: the worst distance of the recovered [s R | t] from the truth, noise-free, over RECOVERY_SEEDS
RECOVERY_SEEDS = (1, 2, 3, 4, 5, 6)
SCIPY_GAP = 7.75e-7                                                        # measured: (stage 2's robust chi2 - scipy's minimum of the same cost) / that minimum


def _ref(s, fix=True, trace=None, th2=10):
    import sim3opt_ref as R
    return R.optimize_sim3(s, th2, fix, trace)


def _host(s, fix=True, th2=10):
    import sim3opt_scene as SC
    return SC.HostOptimizer().OptimizeSim3([s], th2, fix)[0]


@pytest.mark.parametrize("outliers", [0.0, 0.3])
@pytest.mark.parametrize("fix", [True, False])
@pytest.mark.parametrize("n", [10, 33, 65, 129])
def test_host_library_equals_the_restatement_bit_for_bit(n, fix, outliers):
    import sim3opt_scene as SC
    s = SC.scene(n + (50 if fix else 0), n, outliers=outliers, scale=1.0 if fix else 0.93, start=(0.03, 0.03, 0.0 if fix else -0.04))
    g = _host(s, fix)
    SC.assert_same(g, _ref(s, fix), (n, fix, outliers))
    assert g["n_stages"] == (2 if n - g["n_bad"] >= 10 else 1)


def test_defined_exp_against_the_maths_library():
    import sim3opt_ref as R
    import sim3opt_scene as SC
    x = np.concatenate([np.linspace(-1, 1, 200001), [-20.0, -7.3, -2.5, 1.5, 3.25, 10.0, 20.0], np.array([1e-9, -1e-9, 1e-5, -1e-5, 5e-324, 0.34657359027997264, 0.3465735902799727])])
    y = np.zeros_like(x)
    SC.host().sindh_sim3opt_exp(C.c_void_p(x.ctypes.data), len(x), C.c_void_p(y.ctypes.data))
    ref = np.array([math.exp(v) for v in x])
    ulps = int(np.abs(y.view(np.int64) - ref.view(np.int64)).max())
    print("defined exp: largest distance from math.exp in ulps:", ulps)
    assert ulps <= 2 * EXP_ULPS
    z = np.array([0.0, -0.0, np.nan, 710.0, -746.0, np.inf, -np.inf]); w = np.full(7, 5.0)
    SC.host().sindh_sim3opt_exp(C.c_void_p(z.ctypes.data), 7, C.c_void_p(w.ctypes.data))
    assert w[0] == 1.0 and w[1] == 1.0 and np.isnan(w[2]) and w[3] == np.inf and w[4] == 0.0 and w[5] == np.inf and w[6] == 0.0
    with np.errstate(all="ignore"):
        for k in list(range(0, len(x), 4001)) + list(range(len(x) - 14, len(x))):                      # the restatement's is the same function
            assert SC.bits(np.float64(R.exp(x[k]))) == SC.bits(y[k]), x[k]
        assert R.exp(0.0) == 1.0 and np.isnan(R.exp(np.nan))


def _analytic(est, K1, K2, X1, X2):
    """the Jacobians [2, 7] of the two errors for the update Sim3(u) * est at u = 0, u = (omega, upsilon, sigma): -> J12, J21"""
    import sim3opt_scene as SC
    R, t, s = SC.rotation(est[0]) * np.linalg.norm(est[0]) ** 2, np.asarray(est[1], np.float64), float(est[2])      # an unnormalised quaternion rotates and scales by |q|^2
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    dcam = lambda K, p: np.array([[K[0] / p[2], 0, -K[0] * p[0] / p[2] ** 2], [0, K[1] / p[2], -K[1] * p[1] / p[2] ** 2]])
    p = s * R @ X2 + t
    J12 = -dcam(K1, p) @ np.concatenate([-skew(p), np.eye(3), p[:, None]], 1)
    Rinv = np.linalg.inv(s * R)
    p = Rinv @ (X1 - t)
    J21 = -dcam(K2, p) @ (-Rinv @ np.concatenate([-skew(X1), np.eye(3), X1[:, None]], 1))
    return J12, J21


def test_numeric_jacobian_against_the_analytic_one():
    """the restated edges and their central differences with 1e-9, whose floor in FP64 is about 1e-7 of the largest entry"""
    import sim3opt_ref as R
    import sim3opt_scene as SC
    worst = 0.0
    for seed in range(8):
        s = SC.scene(600 + seed, 6, outliers=0, scale=(1.0, 1.3, 0.8)[seed % 3])
        est = R.from_input(s["s12"], s["R12"], s["t12"])
        qts = np.array(list(est[0]) + list(est[1]) + [est[2]], np.float64)
        for i in range(6):
            out = [np.zeros(2), np.zeros((2, 7)), np.zeros(2), np.zeros((2, 7))]
            ptr = lambda a: C.c_void_p(a.ctypes.data)
            f = lambda a: np.ascontiguousarray(a, np.float32)
            args = [f(s["K1"]), f(s["K2"]), f(s["x3Dc1"][i]), f(s["x3Dc2"][i]), f(s["obs1_xy"][i]), f(s["obs2_xy"][i])]
            for fix in (0, 1):
                SC.host().sindh_sim3opt_edges(ptr(qts), fix, *[ptr(a) for a in args], *[ptr(a) for a in out])
                J12, J21 = _analytic(est, s["K1"].astype(np.float64), s["K2"].astype(np.float64), s["x3Dc1"][i].astype(np.float64), s["x3Dc2"][i].astype(np.float64))
                if fix:
                    assert (out[1][:, 6] == 0).all() and (out[3][:, 6] == 0).all() and not np.signbit(out[1][:, 6]).any()      # update[6] = 0: both evaluations are the same
                    continue
                with np.errstate(all="ignore"):                          # and the restatement's numeric Jacobian is the library's
                    TT = [R.perturbed(est, k, False) for k in range(15)]
                    Jr = R.numeric_jacobian([a for a, _ in TT], [np.float64(k) for k in s["K1"]], [np.float64(v) for v in s["x3Dc2"][i]], np.float64(s["obs1_xy"][i, 0]), np.float64(s["obs1_xy"][i, 1]), np.float64(1))
                assert np.array_equal(SC.bits(np.array(Jr, np.float64)), SC.bits(out[1]))
                for Jn, Ja in ((out[1], J12), (out[3], J21)):
                    worst = max(worst, np.abs(Jn - Ja).max() / np.abs(Ja).max())
    print(f"numeric against analytic Jacobian: largest relative deviation {worst:.3e}")
    assert worst <= 4 * JACOBIAN_DEVIATION


@pytest.mark.parametrize("fix", [True, False])
def test_recovers_the_true_sim3_without_noise(fix):
    """no noise, no outliers, the input off by 0.05 rad, 5 cm and (scale free) 5 %.  What is left is the FP32 rounding of the points of camera 1"""
    import sim3opt_scene as SC
    worst = 0.0
    for seed in RECOVERY_SEEDS:
        s = SC.scene(700 + seed, 60, outliers=0, noise=0.0, scale=1.0 if fix else 1.2, start=(0.05, 0.05, 0.0 if fix else 0.05))
        g = _host(s, fix)
        assert g["n_inliers"] == 60 and g["n_stages"] == 2 and not g["removed"].any()
        worst = max(worst, SC.distance(g, s))
        if fix:
            assert g["s"].tobytes() == np.float64(s["s12"]).tobytes()      # s never changes: the bit pattern of the input
    print(f"recovery, fix_scale={fix}: worst distance of [s R | t] from the truth {worst:.3e}")
    assert worst <= 10 * RECOVERY


def _scipy_cost(s, keep, fix, th2=10.0):
    """the minimum scipy finds of the Huber cost of the kept pairs, started at the item's input Sim3"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    delta = float(np.float32(np.sqrt(np.float32(th2))))
    k1, k2 = s["K1"].astype(np.float64), s["K2"].astype(np.float64)
    X1, X2 = s["x3Dc1"][keep].astype(np.float64), s["x3Dc2"][keep].astype(np.float64)
    o1, o2 = s["obs1_xy"][keep].astype(np.float64), s["obs2_xy"][keep].astype(np.float64)
    w1, w2 = np.sqrt(s["inv_sigma2_1"][keep].astype(np.float64)), np.sqrt(s["inv_sigma2_2"][keep].astype(np.float64))
    R0, t0, s0 = s["R12"].astype(np.float64), s["t12"].astype(np.float64), float(s["s12"])

    def res(u):
        sc = s0 * (1.0 if fix else np.exp(u[6]))
        R = Rotation.from_rotvec(u[:3]).as_matrix() @ R0; t = t0 + u[3:6]
        p = sc * X2 @ R.T + t; q = ((X1 - t) @ R) / sc
        e1 = w1[:, None] * (o1 - np.stack([k1[0] * p[:, 0] / p[:, 2] + k1[2], k1[1] * p[:, 1] / p[:, 2] + k1[3]], 1))
        e2 = w2[:, None] * (o2 - np.stack([k2[0] * q[:, 0] / q[:, 2] + k2[2], k2[1] * q[:, 1] / q[:, 2] + k2[3]], 1))
        e = np.concatenate([e1, e2]); r = np.maximum(np.linalg.norm(e, axis=1), 1e-300)
        f = np.where(r <= delta, 1.0, np.sqrt(np.maximum(2 * delta * r - delta * delta, 0)) / r)                  # |f e|^2 is Huber's rho[0] of |e|^2
        return (e * f[:, None]).reshape(-1)
    sol = least_squares(res, np.zeros(7), method="trf", x_scale=1.0, xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
    return float((res(sol.x) ** 2).sum())


@pytest.mark.parametrize("fix", [True, False])
def test_the_second_stage_reaches_the_huber_minimum_scipy_finds(fix):
    """with noise and outliers: stage 2 minimises the Huber cost of the pairs stage 1 left; scipy minimises the same cost from the same start"""
    pytest.importorskip("scipy")
    import sim3opt_scene as SC
    s = SC.scene(65, 65, outliers=0.3, noise=0.5, scale=1.0 if fix else 1.1, start=(0.03, 0.03, 0.0 if fix else 0.03))
    tr = []
    r = _ref(s, fix, tr)
    g = _host(s, fix)
    SC.assert_same(g, r, "scene")
    assert g["n_stages"] == 2
    keep = ~np.array([t for t in tr if t[0] == 0 and t[1] == "classified"][0][2])      # the pairs of stage 2: those stage 1's classification left
    best = _scipy_cost(s, keep, fix)
    gap = (float(g["stage_chi2"][1]) - best) / best
    print(f"fix_scale={fix}: stage 2 robust chi2 {g['stage_chi2'][1]:.9f}, scipy {best:.9f}, gap {gap:.3e}")
    assert gap <= 4 * SCIPY_GAP


@pytest.mark.parametrize("fix", [True, False])
@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_planted_outliers_are_exactly_the_removed_pairs(fix, noise):
    """gross in image 1 only, in image 2 only and in both: `e12->chi2()>th2 || e21->chi2()>th2`"""
    import sim3opt_scene as SC
    n = 81
    s = SC.scene(7, n, outliers=24, noise=noise, scale=1.0 if fix else 1.15)
    assert sorted(set(s["outlier_side"][s["is_outlier"]])) == [0, 1, 2]
    g = _host(s, fix)
    assert np.array_equal(g["removed"].astype(bool), s["is_outlier"])
    assert g["n_bad"] == 24 and g["n_inliers"] == n - 24 and g["n_stages"] == 2


def test_the_second_stage_runs_up_to_ten_iterations_after_removals_and_up_to_five_without():
    import sim3opt_scene as SC
    for seed in range(6):                                               # ordinary scenes: the stop criterion ends either stage early
        for outliers in (0, 0.3):
            g = _host(SC.scene(800 + seed, 40, outliers=outliers))
            assert 1 <= g["stage_iters"][0] <= 5 and 1 <= g["stage_iters"][1] <= (10 if g["n_bad"] else 5) and (g["n_bad"] > 0) == (outliers > 0)
    far = SC.scene(905, 60, outliers=0, noise=0.5, start=(1.2, 2.0, -0.4))      # a start so far off that stage 1 ends unconverged: 48 pairs go, the other 12 need 6 more iterations
    g = _host(far, False)
    SC.assert_same(g, _ref(far, False), "far")
    assert g["n_bad"] > 0 and g["stage_iters"][0] == 5 and 5 < g["stage_iters"][1] <= 10
    nan = SC.depth_zero()                                               # a system of NaNs never meets the stop criterion: nBad == 0 and exactly 5 more
    g = _host(nan)
    assert g["n_bad"] == 0 and list(g["stage_iters"]) == [5, 5]


def test_early_returns_leave_the_sim3_and_keep_the_nulled_matches():
    import sim3opt_scene as SC
    from sindslam_amd.matcher import sim3opt_items
    s = SC.scene(19, 12, outliers=3)                                    # 12 pairs, 3 outliers: 9 < 10 after the first stage
    for fix in (True, False):
        arr, keep = sim3opt_items([s])
        a = keep[0]
        assert SC.host().sindh_sim3_optimize(arr, 1, 10.0, int(fix)) == 0
        empty = _host(dict(s, **{k: s[k][:0] for k in ("x3Dc1", "x3Dc2", "obs1_xy", "obs2_xy", "inv_sigma2_1", "inv_sigma2_2")}), fix)      # n = 0: the input Sim3 as the library holds it
        assert a["n_inliers"][0] == 0 and a["n_stages"][0] == 1 and a["n_bad"][0] == 3 and np.array_equal(a["removed"].astype(bool), s["is_outlier"])
        assert a["q_out"].tobytes() == empty["q"].tobytes() and a["t_out"].tobytes() == empty["t"].tobytes() and a["s_out"].tobytes() == np.float64(s["s12"]).tobytes()
        assert a["t_out"].tobytes() == s["t12"].astype(np.float64).tobytes() and a["stage_iters"][0] >= 1 and a["stage_iters"][1] == 0
        assert empty["n_inliers"] == 0 and empty["n_stages"] == 0 and empty["n_bad"] == 0 and (empty["stage_iters"] == 0).all() and len(empty["removed"]) == 0
        SC.assert_same(empty, _ref(dict(s, **{k: s[k][:0] for k in ("x3Dc1", "x3Dc2", "obs1_xy", "obs2_xy", "inv_sigma2_1", "inv_sigma2_2")}), fix), "n = 0")
        nine = SC.scene(9, 9, outliers=0)
        g = _host(nine, fix)
        SC.assert_same(g, _ref(nine, fix), "n = 9")
        assert g["n_inliers"] == 0 and g["n_stages"] == 1 and not g["removed"].any() and g["t"].tobytes() == nine["t12"].astype(np.float64).tobytes()
        ten = SC.scene(10, 10, outliers=0)
        assert _host(ten, fix)["n_stages"] == 2 and _host(ten, fix)["n_inliers"] == 10      # nCorrespondences - nBad < 10 is the only way out


@pytest.mark.parametrize("fix", [True, False])
def test_degenerate_scenes_return_and_equal_the_restatement(fix):
    import sim3opt_scene as SC
    d = SC.degenerates()
    tr = {k: [] for k in d}
    got = {k: _host(s, fix) for k, s in d.items()}
    for k, s in d.items():
        SC.assert_same(got[k], _ref(s, fix, tr[k]), k)
    trials = [t for t in tr["depth_zero"] if len(t) == 5]               # a point at depth 0: the system is NaN, every step is rejected, the NaN errors classify nothing
    assert trials and all(not t[4] and not np.isfinite(t[3]) for t in trials) and not got["depth_zero"]["removed"].any()
    assert got["depth_zero"]["t"].tobytes() == d["depth_zero"]["t12"].astype(np.float64).tobytes() and np.isfinite(got["depth_zero"]["q"]).all()
    g = got["identical_points"]                                         # rank-deficient H: lambda carries the solve
    assert g["n_stages"] == 2 and np.isfinite(g["q"]).all() and np.isfinite(g["t"]).all() and np.isfinite(g["stage_chi2"]).all()
    g = got["exact_identity"]                                           # every error is 0: rho == 0 terminates after one iteration
    assert list(g["stage_iters"]) == [1, 1] and (g["stage_chi2"] == 0).all() and g["n_inliers"] == 12 and g["q"].tobytes() == np.array([0, 0, 0, 1.0]).tobytes() and (g["t"] == 0).all() and g["s"] == 1.0


def test_a_sanitizer_build_of_the_host_twin_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_sim3_optimize and csrc/host/sim3_opt.cpp with -fsanitize=address,undefined, run as a program of its own on the scenes of this file"""
    import sim3opt_scene as SC
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "sim3opt_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "sindslam_amd", "csrc"), "sanitize-sim3opt", "OUT=" + exe], check=True, capture_output=True, text=True)
    scenes = [(SC.scene(n + (50 if fix else 0), n, outliers=o, scale=1.0 if fix else 0.93, start=(0.03, 0.03, 0.0 if fix else -0.04)), fix) for n in (10, 33, 65, 129) for fix in (True, False) for o in (0.0, 0.3)]
    scenes += [(s, fix) for s in SC.degenerates().values() for fix in (True, False)]
    scenes += [(SC.scene(19, 12, outliers=3), True), (SC.scene(9, 9, outliers=0), False), (SC.scene(2, 0, outliers=0), True), (SC.scene(905, 60, outliers=0, start=(1.2, 2.0, -0.4)), False)]
    with open(tmp_path / "items.bin", "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for s, fix in scenes:
            n = len(s["inv_sigma2_1"])
            f.write(np.array([n, int(fix)], np.int32).tobytes()); f.write(np.array([10.0, s["s12"]], np.float32).tobytes())
            for k in ("K1", "K2", "R12", "t12", "x3Dc1", "x3Dc2", "obs1_xy", "obs2_xy", "inv_sigma2_1", "inv_sigma2_2"):
                f.write(np.ascontiguousarray(s[k], np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "items.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(scenes)
    for line, (s, fix) in zip(lines, scenes):                           # and it computed what the library computes
        g = _host(s, fix)
        assert [int(v) for v in line.split()] == [g["n_inliers"], g["n_bad"], g["n_stages"], int(g["removed"].sum()), int(np.float64(g["s"]).view(np.uint64))]


# ---------------------------------------------------------------- the Python layer (sindslam_amd/optimizer.py) on toys, with the host twin in the device's place
def _toy_key_frames(n=40, seed=3, outliers=0):
    """two key frames of N slots whose map points are the pairs of a scene, in shuffled slots, among slots that are empty, bad or unmatched -> kf1, kf2, vpMatches1, scene"""
    import sim3opt_scene as SC
    s = SC.scene(seed, n, outliers=outliers, noise=0.3)
    rng = np.random.default_rng(seed)
    N1, N2 = n + 9, n + 5
    slot1 = np.sort(rng.choice(N1, n, replace=False)); slot2 = rng.permutation(N2)[:n]
    T1 = np.eye(4, dtype=np.float32); T2 = np.eye(4, dtype=np.float32); T2[:3, 3] = (0.5, -0.25, 0.125)      # x3Dw2 = x3Dc2 - t comes back as x3Dc2 exactly for the pairs in `keep`, within an ulp for the others
    def kf(N, slot, X, obs, inv, K, T):
        k = dict(un_xy=np.zeros((N, 2), np.float32), inv_sigma2=np.ones(N, np.float32), mp=np.full(N, -1, np.int64), x3Dw=np.zeros((N, 3), np.float32), bad=np.zeros(N, np.uint8), Tcw=T, K=K)
        k["un_xy"][slot] = obs; k["inv_sigma2"][slot] = inv; k["mp"][slot] = 100 + np.arange(len(slot)); k["x3Dw"][slot] = X
        return k
    X2w = (s["x3Dc2"].astype(np.float64) - T2[:3, 3]).astype(np.float32)
    keep = np.array([np.array_equal((X2w[i].astype(np.float32) + T2[:3, 3]).astype(np.float32), s["x3Dc2"][i]) for i in range(n)])
    kf1 = kf(N1, slot1, s["x3Dc1"], s["obs1_xy"], s["inv_sigma2_1"], s["K1"], T1); kf2 = kf(N2, slot2, X2w, s["obs2_xy"], s["inv_sigma2_2"], s["K2"], T2)
    m = np.full(N1, -1, np.int32); m[slot1] = slot2
    return kf1, kf2, m, s, slot1, slot2, keep


def test_sim3_item_flattens_as_the_reference_and_maps_the_rows_back():
    import sim3opt_scene as SC
    from sindslam_amd.optimizer import OptimizeSim3, sim3_item
    kf1, kf2, m, s, slot1, slot2, keep = _toy_key_frames(outliers=6)
    kf1["mp"][slot1[3]] = -1                                            # pMP1 NULL: skipped (:1112)
    kf1["bad"][slot1[5]] = 1; kf2["bad"][slot2[8]] = 1                 # either bad: skipped (:1114)
    m[slot1[11]] = -1                                                   # no match (:1101)
    gone = np.zeros(len(slot1), bool); gone[[3, 5, 8, 11]] = True
    item, idx = sim3_item(kf1, kf2, m, s["s12"], s["R12"], s["t12"])
    assert np.array_equal(idx, slot1[~gone]) and len(item["inv_sigma2_1"]) == len(slot1) - 4
    rows = np.nonzero(~gone)[0]
    assert np.array_equal(item["x3Dc1"], s["x3Dc1"][rows]) and np.array_equal(item["obs2_xy"], s["obs2_xy"][rows]) and np.array_equal(item["inv_sigma2_2"], s["inv_sigma2_2"][rows])
    assert np.array_equal(item["x3Dc2"][keep[rows]], s["x3Dc2"][rows][keep[rows]]) and keep.sum() > 10 and np.abs(item["x3Dc2"] - s["x3Dc2"][rows]).max() < 1e-6      # R2w * P3D2w + t2w in FP32
    nIn, m2, S12 = OptimizeSim3(SC.HostOptimizer(), kf1, kf2, m, s["s12"], s["R12"], s["t12"], 10, True)
    direct = SC.HostOptimizer().OptimizeSim3([item], 10, True)[0]
    assert nIn == direct["n_inliers"] >= 20 and S12["q"].tobytes() == direct["q"].tobytes()
    nulled = np.nonzero((m >= 0) & (m2 < 0))[0]
    assert np.array_equal(nulled, idx[direct["removed"].astype(bool)]) and np.array_equal(np.isin(slot1, nulled), s["is_outlier"] & ~gone)
    assert np.array_equal(m2[m2 >= 0], m[m2 >= 0]) and m2[slot1[3]] == m[slot1[3]]      # a skipped pair's match is not touched


def test_loop_scw_is_the_product_with_the_key_frames_pose():
    import sim3opt_scene as SC
    from sindslam_amd.optimizer import loop_scw
    s = SC.scene(5, 30, outliers=0, scale=1.1)
    g = _host(s, False)
    rng = np.random.default_rng(1)
    R, t = SC.S.pose(rng)
    T = np.eye(4, dtype=np.float32); T[:3, :3] = R; T[:3, 3] = t
    Scw, gS = loop_scw(g, T)
    ref = np.eye(4); ref[:3, :3] = float(g["s"]) * SC.rotation(g["q"]) @ T[:3, :3].astype(np.float64); ref[:3, 3] = float(g["s"]) * SC.rotation(g["q"]) @ T[:3, 3].astype(np.float64) + g["t"]
    assert Scw.dtype == np.float32 and np.abs(Scw - ref).max() < 2e-6 and (Scw[3] == (0, 0, 0, 1)).all()
    assert gS["s"] == g["s"] and abs(np.linalg.norm(gS["q"]) - 1) < 1e-6
    I, gI = loop_scw(dict(q=[0, 0, 0, 1.0], t=[1, 2, 3.0], s=2.0), np.eye(4))
    assert np.array_equal(I, np.array([[2, 0, 0, 1], [0, 2, 0, 2], [0, 0, 2, 3], [0, 0, 0, 1]], np.float32))


class _ToyMatcher:
    """SearchBySim3 and SearchByProjectionSim3 scripted, OptimizeSim3 the host twin's"""

    def __init__(self, add12=(), add_proj=()):
        import sim3opt_scene as SC
        self.add12, self.add_proj, self.calls, self.host = add12, add_proj, [], SC.HostOptimizer()

    def SearchBySim3(self, pairs, th):
        (T1, T2, s12, R12, t12, s1, s2), = pairs
        self.calls.append(("sim3", th, s1["valid"].copy(), s2["valid"].copy()))
        m = np.full(len(s1["valid"]), -1, np.int32)
        for i1, i2 in self.add12:
            assert s1["valid"][i1] and s2["valid"][i2]
            m[i1] = i2
        return [(m, len(self.add12))]

    def OptimizeSim3(self, items, th2=10, fix_scale=True):
        self.calls.append(("optimize", th2, fix_scale, len(items[0]["inv_sigma2_1"])))
        return self.host.OptimizeSim3(items, th2, fix_scale)

    def SearchByProjectionSim3(self, items, th):
        (Scw, mp, kf), = items
        self.calls.append(("proj", th, mp["valid"].copy(), kf["taken"].copy(), Scw.copy()))
        m = np.full(len(kf["taken"]), -1, np.int32)
        for slot, point in self.add_proj:
            assert mp["valid"][point] and not kf["taken"][slot]
            m[slot] = point
        return [(m, len(self.add_proj))]


class _ToySolver:
    def __init__(self, s):
        self.s = s

    def GetEstimatedRotation(self): return self.s["R12"]
    def GetEstimatedTranslation(self): return self.s["t12"]
    def GetEstimatedScale(self): return self.s["s12"]


def test_compute_sim3_accept_searches_optimises_and_asks_for_twenty_inliers():
    from sindslam_amd.optimizer import compute_sim3_accept, loop_scw
    kf1, kf2, m, s, slot1, slot2, keep = _toy_key_frames(n=40, outliers=0)
    for k in (kf1, kf2):
        k.update(max_dist=None, min_dist=None, mp_desc=None, octave=None, kf_desc=None, grid_start=None, grid_idx=None)
    given = np.zeros(len(slot1), bool); given[:30] = True                # SearchByBoW matched 30 pairs; RANSAC calls 16 of them inliers, 25 in the second case
    match12 = np.full(len(m), -1, np.int32); match12[slot1[given]] = slot2[given]
    for n_ransac, n_added, verdict in ((16, 0, False), (16, 6, True), (25, 0, True)):
        vb = np.zeros(len(m), bool); vb[slot1[:n_ransac]] = True
        add = [(int(slot1[30 + k]), int(slot2[30 + k])) for k in range(n_added)]
        toy = _ToyMatcher(add12=add); trace = []
        accept = compute_sim3_accept(toy, kf1, [None, dict(kf=kf2, match12=match12)], [None, _ToySolver(s)], True, trace=trace)
        assert accept(1, None, vb) is verdict
        assert [c[0] for c in toy.calls] == ["sim3", "optimize"] and toy.calls[0][1] == 7.5 and toy.calls[1][1:] == (10, True, n_ransac + n_added)
        v1, v2 = toy.calls[0][2].astype(bool), toy.calls[0][3].astype(bool)                                      # vbAlreadyMatched1 / 2: the RANSAC inliers only
        assert not v1[slot1[:n_ransac]].any() and v1[slot1[n_ransac:]].all() and not v2[slot2[:n_ransac]].any() and v2[slot2[n_ransac:40]].all() and not v1[kf1["mp"] < 0].any()
        assert trace == [("search_by_sim3", 1, n_added, n_ransac + n_added), ("optimize_sim3", 1, n_ransac + n_added)]
        st = accept.state
        if verdict:
            assert st["matched"] == 1 and int((st["vpMatches"] >= 0).sum()) == n_ransac + n_added and np.array_equal(st["Scw"], loop_scw(st["S12"], kf2["Tcw"])[0])
        else:
            assert st == {}


def test_loop_accept_gathers_the_loop_points_once_and_counts_forty():
    from sindslam_amd.optimizer import loop_accept
    N = 60
    def kf(ids, bad=()):
        k = dict(mp=np.array(ids, np.int64), bad=np.isin(np.arange(len(ids)), bad).astype(np.uint8), x3Dw=np.zeros((len(ids), 3), np.float32), normal=np.zeros((len(ids), 3), np.float32),
                 max_dist=np.ones(len(ids), np.float32), min_dist=np.ones(len(ids), np.float32), mp_desc=np.zeros((len(ids), 32), np.uint8))
        k["x3Dw"][:, 0] = k["mp"]
        return k
    loop_kfs = [kf([1, 2, -1, 3, 4], bad=[3]), kf([2, 5, 6] + list(range(100, 130))), kf([3, 1, 7])]      # 3 is bad in the first and good in the last
    matched = np.full(N, -1, np.int64); matched[:35] = [5, 100] + list(range(200, 233))
    kf1 = dict(un_xy=np.zeros((N, 2), np.float32), octave=np.zeros(N, np.int32), kf_desc=np.zeros((N, 32), np.uint8), grid_start=None, grid_idx=None)
    Scw = np.eye(4, dtype=np.float32)
    for extra, verdict in ((4, False), (5, True)):
        toy = _ToyMatcher(add_proj=[(40 + k, (4, 6, 7, 8, 9)[k]) for k in range(extra)])      # rows of the list that hold the ids 6, 101, 102, 103, 104
        ok, total, out, ids = loop_accept(toy, kf1, Scw, loop_kfs, matched)
        assert list(ids) == [1, 2, 4, 5, 6] + list(range(100, 130)) + [3, 7]
        call, = toy.calls
        assert call[1] == 10 and np.array_equal(call[2].astype(bool), ~np.isin(ids, [5, 100])) and np.array_equal(call[3].astype(bool), matched >= 0)
        assert ok is verdict and total == 35 + extra and np.array_equal(out[:35], matched[:35]) and list(out[40:40 + extra]) == [6, 101, 102, 103, 104][:extra]
