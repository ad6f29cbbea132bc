"""CPU: the host twin of sind_match_local_ba (sindh_local_ba; csrc/host/local_ba.hpp, csrc/host/local_ba.cpp) against the Python restatement tests/localba_ref.py, bit
for bit; the Schur path against a dense solve of the full system; the analytic Jacobians against central differences of a projection written here; stage 2 against
scipy's minimum of the same cost, which shares nothing with the code under test; planted outliers; the literal and degenerate cases; the error paths; a stand-alone
sanitizer build; and the graph collection of sindslam_amd/optimizer.py on a toy map.  The measured figures named below are in profiles/match_local_ba.txt."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
SCHUR_DEVIATION = 1.06e-13                                               # measured: |x - numpy's solve of the full (6P + 3M) system| / |x|, the largest over the scenes below
JACOBIAN_DEVIATION = 6.43e-10                                            # measured: analytic against central differences, relative to the largest entry of the edge's Jacobian
SCIPY_GAP = 1.23e-5                                                     # measured: (stage 2's chi2 - scipy's minimum of the same cost) / that minimum; the stop criterion ends a stage after three steps that gain under 1e-3
LBA_C = 56                                                              # doubles per edge of csrc/host/ba_schur.hpp


def _host(s):
    import localba_scene as SC
    return SC.HostBA().LocalBundleAdjustment([s])[0]


def _ref(s):
    import localba_ref as R
    import localba_scene as SC
    return R.local_ba(s, SC.K5)


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("seed", [2, 21])
def test_host_library_equals_the_restatement_bit_for_bit(kind, seed):
    """4 key frames x 30 points; seed 21: key frame id 0 among them, 3 of 4 key frames per point, ids shuffled"""
    import localba_scene as SC
    s = SC.scene(seed, 3, 1, 30, kind=kind, outliers=4, obs_per_point=3 if seed == 21 else None, id0=seed == 21)
    g = _host(s)
    SC.assert_same(g, _ref(s), (kind, seed))
    assert g["n_stages"] == 2 and g["n_level1"] >= 4


def _full_system(s, Cc, lam):
    """the full (6P + 3M) system of the first linearisation from the edges' contributions, lambda on the diagonal -> H, b"""
    free = sorted([k for k in range(len(s["kf_id"])) if s["kf_kind"][k] == 0], key=lambda k: int(s["kf_id"][k]))
    rank = {k: i for i, k in enumerate(free)}
    P, M = len(free), len(s["mp_id"])
    H = np.zeros((6 * P + 3 * M, 6 * P + 3 * M)); b = np.zeros(6 * P + 3 * M)
    iu6, iu3 = np.triu_indices(6), np.triu_indices(3)
    for j in range(M):
        for e in range(s["obs_start"][j], s["obs_start"][j + 1]):
            c = Cc[e]; o = 6 * P + 3 * j
            Hl = np.zeros((3, 3)); Hl[iu3] = c[27:33]; Hl = Hl + np.triu(Hl, 1).T
            H[o:o + 3, o:o + 3] += Hl; b[o:o + 3] += c[33:36]
            k = int(s["obs_kf"][e])
            if k in rank:
                i = 6 * rank[k]
                Hp = np.zeros((6, 6)); Hp[iu6] = c[0:21]; Hp = Hp + np.triu(Hp, 1).T
                H[i:i + 6, i:i + 6] += Hp; b[i:i + 6] += c[21:27]
                H[i:i + 6, o:o + 3] += c[36:54].reshape(6, 3); H[o:o + 3, i:i + 6] += c[36:54].reshape(6, 3).T
    return H + lam * np.eye(len(b)), b


def test_schur_path_solves_the_full_system():
    """the first linearisation of a scene: x of the Schur complement, the dense LDL^T and the back-substitution against numpy's solve of the whole system"""
    import localba_scene as SC
    worst = 0.0
    for seed, kind in ((31, "mono"), (32, "stereo"), (33, "mixed"), (34, "mixed")):
        s = SC.scene(seed, 4, 1, 30, kind=kind, outliers=3, obs_per_point=None if seed < 34 else 3)
        from sindslam_amd.matcher import localba_items
        arr, keep = localba_items([s])
        n_obs, P, M = len(s["obs_kf"]), int((s["kf_kind"] == 0).sum()), len(s["mp_id"])
        Cc = np.zeros((n_obs, LBA_C)); x = np.zeros(6 * P + 3 * M); lam = np.zeros(1)
        K = np.ascontiguousarray(SC.K5)
        SC.host().sindh_localba_linear.argtypes = [C.c_void_p] * 5
        assert SC.host().sindh_localba_linear(C.addressof(arr), K.ctypes.data, Cc.ctypes.data, x.ctypes.data, lam.ctypes.data) == 0
        H, b = _full_system(s, Cc, lam[0])
        ref = np.linalg.solve(H, b)
        worst = max(worst, np.linalg.norm(x - ref) / np.linalg.norm(ref))
        assert lam[0] > 0 and np.linalg.norm(ref) > 1e-3
    print(f"Schur path against numpy's solve of the full system: largest relative deviation {worst:.3e}")
    assert worst <= 4 * SCHUR_DEVIATION


def _project(T, X, K, stereo, float_invz=False):
    """float_invz: the stereo edge's `const float invz`, which makes the library's cost a slightly different (and not smooth) function"""
    p = T[:3, :3] @ X + T[:3, 3]
    if stereo and float_invz:
        iz = np.float64(np.float32(1.0 / p[2])); u = p[0] * iz * K[0] + K[2]
        return np.array([u, p[1] * iz * K[1] + K[3], u - K[4] * iz])
    u = K[0] * p[0] / p[2] + K[2]; v = K[1] * p[1] / p[2] + K[3]
    return np.array([u, v, u - K[4] / p[2]]) if stereo else np.array([u, v, 0.0])


def _exp_se3(u):
    """SE3 exponential of (omega, upsilon) as a 4 x 4, from its series"""
    A = np.zeros((4, 4)); w = u[:3]
    A[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]; A[:3, 3] = u[3:]
    E = np.eye(4); term = np.eye(4)
    for k in range(1, 12):
        term = term @ A / k; E = E + term
    return E


def test_analytic_jacobians_against_central_differences():
    """_jacobianOplusXi and _jacobianOplusXj of both edges against central differences (h = 1e-6) of error = obs - projection written here in FP64 throughout"""
    import localba_scene as SC
    import poseopt_ref as PR
    SC.host().sindh_localba_edge.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 2
    K = SC.K5.astype(np.float64); worst = 0.0; h = 1e-6
    for seed in range(6):
        s = SC.scene(40 + seed, 3, 1, 6, kind="mixed")
        for e in range(len(s["obs_kf"])):
            k = int(s["obs_kf"][e]); j = int(np.searchsorted(s["obs_start"], e, side="right") - 1)
            q, t = PR.from_tcw(s["Tcw"][k])
            qt = np.array(list(q) + list(t), np.float64); X = s["x3Dw"][j].astype(np.float64)
            ob = np.array([s["obs_xy"][e, 0], s["obs_xy"][e, 1], s["u_right"][e], s["inv_sigma2"][e]], np.float32)
            c = np.zeros(LBA_C); jac = np.zeros(30); K32 = np.ascontiguousarray(SC.K5)
            SC.host().sindh_localba_edge(qt.ctypes.data, X.ctypes.data, ob.ctypes.data, K32.ctypes.data, 0, c.ctypes.data, jac.ctypes.data)
            stereo = not ob[2] < 0
            T = np.eye(4); T[:3, :3] = np.array(PR.quat_to_matrix(q), np.float64); T[:3, 3] = t
            err = lambda T, X: np.array([ob[0], ob[1], ob[2] if stereo else 0.0], np.float64) - _project(T, X, K, stereo)
            Ji = np.stack([(err(T, X + h * d) - err(T, X - h * d)) / (2 * h) for d in np.eye(3)], 1)
            Jj = np.stack([(err(_exp_se3(h * d) @ T, X) - err(_exp_se3(-h * d) @ T, X)) / (2 * h) for d in np.eye(6)], 1)
            A, B = jac[:9].reshape(3, 3), jac[9:27].reshape(3, 6)
            worst = max(worst, np.abs(A - Ji).max() / np.abs(Ji).max(), np.abs(B - Jj).max() / np.abs(Jj).max())
            if not stereo:
                assert (A[2] == 0).all() and (B[2] == 0).all()
    print(f"analytic against numeric Jacobians: largest relative deviation {worst:.3e}")
    assert worst <= 4 * JACOBIAN_DEVIATION


def test_stage_2_reaches_the_minimum_that_scipy_finds():
    """stage 2 has no robust kernel: its chi2 against scipy.optimize.least_squares' minimum of the same cost over the same level-0 edges (the first classification is
    the erase output of the same item with do_more = 0, whose poses and points are the start), the projection written here.  scipy minimises the smooth cost; the
    comparison is at its minimiser with the stereo edge's float invz, which moves the cost by about 4e-7 of itself"""
    optimize = pytest.importorskip("scipy.optimize")
    import localba_scene as SC
    import poseopt_ref as PR
    K = SC.K5.astype(np.float64); worst = 0.0
    for seed, kind in ((51, "mono"), (52, "stereo"), (53, "mixed")):
        s = SC.scene(seed, 3, 1, 14, kind=kind, outliers=2)
        g = _host(s); st1 = _host(dict(s, do_more=False))
        lvl0 = np.nonzero(st1["erase"] == 0)[0]
        assert g["n_stages"] == 2 and g["n_level1"] == int(st1["erase"].sum())
        free = [k for k in range(len(s["kf_id"])) if s["kf_kind"][k] == 0]
        pt = np.repeat(np.arange(len(s["mp_id"])), np.diff(s["obs_start"]))
        T0 = st1["Tcw"].astype(np.float64); X0 = st1["x3Dw"].astype(np.float64)
        for k in range(len(T0)):                                        # the rotation the library holds: the FP32 matrix through the normalised quaternion
            q, t = PR.from_tcw(st1["Tcw"][k]); T0[k, :3, :3] = np.array(PR.quat_to_matrix(q), np.float64)

        def residuals(p, float_invz=False):
            T = T0.copy()
            for i, k in enumerate(free):
                T[k] = _exp_se3(p[6 * i:6 * i + 6]) @ T0[k]
            X = X0 + p[6 * len(free):].reshape(-1, 3)
            r = []
            for e in lvl0:
                stereo = not s["u_right"][e] < 0
                d = np.array([s["obs_xy"][e, 0], s["obs_xy"][e, 1], s["u_right"][e] if stereo else 0.0], np.float64) - _project(T[s["obs_kf"][e]], X[pt[e]], K, stereo, float_invz)
                r.extend(np.sqrt(np.float64(s["inv_sigma2"][e])) * d[:3 if stereo else 2])
            return np.array(r)

        sol = optimize.least_squares(residuals, np.zeros(6 * len(free) + X0.size), method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=200)
        best = float((residuals(sol.x, True) ** 2).sum())              # the library's cost at scipy's minimiser of the smooth one
        gap = (g["stage_chi2"][1] - best) / best
        print(f"{kind}: stage 2 chi2 {g['stage_chi2'][1]:.9f}, scipy's minimum {best:.9f}, gap {gap:.3e}")
        worst = max(worst, gap)
        assert gap > -1e-6                                              # scipy stops within its own tolerances of the minimum: it is not undercut by more than that
    assert worst <= 4 * SCIPY_GAP


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_planted_outliers_are_exactly_the_erased_set(kind):
    """noise 0.5 px, outliers displaced by 20 to 40 px on points with 8 observations, one per point: host twin and restatement both erase exactly those"""
    import localba_scene as SC
    s = SC.scene(7, 6, 2, 30, kind=kind, outliers=5)
    assert s["planted"].sum() == 5
    for r in (_host(s), _ref(s)):
        assert np.array_equal(r["erase"], s["planted"]) and r["n_level1"] == 5 and r["n_stages"] == 2
    g = _host(s)
    assert SC.mean_reprojection_error(g["Tcw"], g["x3Dw"], s, 1 - g["erase"]) < 0.5 * np.sqrt(np.pi / 2) < SC.mean_reprojection_error(s["Tcw"], s["x3Dw"], s, 1 - s["planted"])


def test_literal_and_degenerate_cases():
    import localba_scene as SC
    import poseopt_ref as PR
    cases = SC.literal_cases()
    res = {}
    for name, it in cases.items():
        res[name] = _host(it)
        SC.assert_same(res[name], _ref(it), name)
        assert np.isfinite(res[name]["Tcw"]).all() and np.isfinite(res[name]["x3Dw"]).all(), name
    stop = lambda name: _host(dict(cases[name], do_more=False))
    # a single monocular observation: Hll has rank 2 and is inverted only through lambda; the point moves along with its one edge and stays finite
    g = res["single_mono"]
    assert g["n_stages"] == 2 and g["erase"][-1] == 0 and not np.array_equal(g["x3Dw"][-1], cases["single_mono"]["x3Dw"][-1])
    # a point whose edges all go to level 1 is inactive in stage 2: it keeps the estimate that stage 1 left, bit for bit, while the others move on
    g = res["point_all_level1"]; g1 = stop("point_all_level1")
    assert (g["erase"][-3:] == 1).all() and g["n_level1"] == 3 and g["x3Dw"][-1].tobytes() == g1["x3Dw"][-1].tobytes() and g["x3Dw"][0].tobytes() != g1["x3Dw"][0].tobytes()
    # a local key frame whose edges all go to level 1: P shrinks from 3 to 2 between the stages, the indices close up, its pose stays what stage 1 left
    it = cases["kf_all_level1"]; g = res["kf_all_level1"]; g1 = stop("kf_all_level1")
    of2 = it["obs_kf"] == 2
    assert g["erase"][of2].all() and g["n_stages"] == 2 and g["Tcw"][2].tobytes() == g1["Tcw"][2].tobytes() and g["Tcw"][0].tobytes() != g1["Tcw"][0].tobytes() and g["Tcw"][1].tobytes() != g1["Tcw"][1].tobytes()
    # key frame id 0, local and fixed: its output is the round trip of its input through the quaternion
    it = cases["id0"]; g = res["id0"]
    assert it["kf_kind"][0] == 1 and np.array_equal(SC.bits(g["Tcw"][0]), SC.bits(PR.to_tcw(PR.from_tcw(it["Tcw"][0])))) and g["Tcw"][3].tobytes() == it["Tcw"][3].tobytes()
    # a point behind its cameras, seen exactly where it projects: chi2 is small, isDepthPositive alone sends its edges to level 1 and erases them
    g = res["behind"]
    assert (g["erase"][-3:] == 1).all() and g["erase"][:-3].sum() == 0 and g["n_level1"] == 3
    # a point at depth 0 in a fixed camera: an infinite chi2, every step of stage 1 rejected (one trial each: rho is NaN), the estimates stay the input's round trip;
    # the edge goes to level 1 by its depth and stage 2 runs without it
    it = cases["depth0"]; g = res["depth0"]; g1 = res["depth0_stop"]
    assert np.isinf(g["stage_chi2"][0]) and list(g1["stage_iters"]) == [5, 0] and g1["n_stages"] == 1 and g["n_stages"] == 2 and np.isfinite(g["stage_chi2"][1])
    assert all(np.array_equal(SC.bits(g1["Tcw"][k]), SC.bits(PR.to_tcw(PR.from_tcw(it["Tcw"][k])))) for k in range(3)) and g1["x3Dw"].tobytes() == it["x3Dw"].tobytes()
    assert g1["erase"][it["obs_start"][-2]] == 1
    # do_more = 0: one stage, no level changes, the classification still reported
    g = res["do_more0"]
    assert g["n_stages"] == 1 and g["n_level1"] == 0 and g["stage_iters"][1] == 0 and g["erase"].sum() >= 3
    # n_obs = 0 and n_mp = 0: nothing is optimised, the outputs are the conversions alone
    for name in ("n_obs0", "n_mp0"):
        it = cases[name]; g = res[name]
        assert g["n_stages"] == 0 and g["x3Dw"].tobytes() == it["x3Dw"].tobytes() and g["Tcw"][3].tobytes() == it["Tcw"][3].tobytes()
        assert all(np.array_equal(SC.bits(g["Tcw"][k]), SC.bits(PR.to_tcw(PR.from_tcw(it["Tcw"][k])))) for k in range(3))
    assert SC.HostBA().LocalBundleAdjustment([]) == []


def test_error_paths_write_nothing():
    import localba_scene as SC
    from sindslam_amd.matcher import localba_items
    K = np.ascontiguousarray(SC.K5)
    good = SC.scene(601, 3, 1, 8, kind="mixed")
    for name, bad in SC.bad_items().items():
        arr, keep = localba_items([good, bad])
        for a in keep:
            a["Tcw_out"][:] = 7.0; a["x3Dw_out"][:] = 7.0; a["erase"][:] = 7
        assert SC.host().sindh_local_ba(arr, 2, K.ctypes.data) == SIND_E_ARG, name
        for a in keep:
            assert (a["Tcw_out"] == 7.0).all() and (a["x3Dw_out"] == 7.0).all() and (a["erase"] == 7).all(), name
    arr, keep = localba_items([good])
    for field in ("kf_id", "Tcw", "x3Dw", "obs_start", "obs_kf", "u_right", "erase", "Tcw_out"):      # a NULL array with a non-zero count
        old = getattr(arr[0], field); setattr(arr[0], field, None)
        assert SC.host().sindh_local_ba(arr, 1, K.ctypes.data) == SIND_E_ARG, field
        setattr(arr[0], field, old)
    assert SC.host().sindh_local_ba(arr, 1, K.ctypes.data) == 0
    assert SC.host().sindh_local_ba(None, 1, K.ctypes.data) == SIND_E_ARG and SC.host().sindh_local_ba(arr, -1, K.ctypes.data) == SIND_E_ARG
    for n_local, n_fixed in ((257, 0), (2, 4095)):                      # one free pose, one key frame beyond the limits LBA_MAX_POSES, LBA_MAX_KF
        SC.HostBA().LocalBundleAdjustment([SC.scene(602, n_local, n_fixed, 2, kind="mono", obs_per_point=2)], rc=SIND_E_CAPACITY)


def test_graph_collection_on_a_toy_map():
    """:455-504 by hand.  Key frames 0..5; 3 is the current one, its covisible list is [4, 2, 1] of which 2 is bad.  Points 10..15."""
    from sindslam_amd import optimizer as O

    def kf(mp, covisible=(), bad=False):
        n = len(mp)
        return dict(Tcw=np.eye(4, dtype=np.float32), un_xy=np.arange(2 * n, dtype=np.float32).reshape(n, 2), u_right=np.array([-1.0, 5.0] * n, np.float32)[:n], inv_sigma2=np.full(n, 0.5, np.float32),
                    mp=np.array(mp, np.int64), covisible=list(covisible), bad=bad)

    kfs = {0: kf([12, 13]), 1: kf([-1, 11, 14]), 2: kf([10, 11], bad=True), 3: kf([11, -1, 10, 15], covisible=[4, 2, 1]), 4: kf([12, 10, 13]), 5: kf([14, 16])}
    mps = {10: dict(x3Dw=[0, 0, 5], obs={3: 2, 2: 0, 4: 1}), 11: dict(x3Dw=[1, 0, 5], obs={3: 0, 2: 1, 1: 1}), 12: dict(x3Dw=[2, 0, 5], obs={4: 0, 0: 0}), 13: dict(x3Dw=[3, 0, 5], obs={4: 2, 0: 1}, bad=True),
           14: dict(x3Dw=[4, 0, 5], obs={1: 2, 5: 0}), 15: dict(x3Dw=[5, 0, 5], obs={3: 3}), 16: dict(x3Dw=[6, 0, 5], obs={5: 1})}
    local, points, fixed, item = O.local_ba_graph(3, kfs, mps)
    assert local == [3, 4, 1]                                           # the bad neighbour 2 is left out
    assert points == [11, 10, 15, 12, 14]                               # in the order the local key frames hold them; 13 is bad, 16 is seen by no local key frame
    assert fixed == [0, 5]                                              # 2 sees points 11 and 10 but carries the local mark (and is bad); 0 through 12, 5 through 14
    assert list(item["kf_id"]) == [3, 4, 1, 0, 5] and list(item["kf_kind"]) == [0, 0, 0, 2, 2]
    assert item["pairs"] == [(1, 11), (3, 11), (3, 10), (4, 10), (3, 15), (0, 12), (4, 12), (1, 14), (5, 14)]      # ascending key-frame id per point, the bad key frame 2 skipped
    assert list(item["obs_start"]) == [0, 2, 4, 5, 7, 9] and list(item["obs_kf"]) == [2, 0, 0, 1, 0, 3, 1, 2, 4]
    assert list(item["u_right"]) == [5.0, -1.0, -1.0, 5.0, 5.0, -1.0, -1.0, -1.0, -1.0] and item["obs_xy"][2].tolist() == [4.0, 5.0]
    kfs[0], kfs[9] = kf([12]), kf([12, 13])                             # key frame 0 as a neighbour is local and fixed
    kfs[3]["covisible"] = [0]
    local, points, fixed, item = O.local_ba_graph(3, kfs, mps)
    assert local == [3, 0] and list(item["kf_kind"][:2]) == [0, 1]

    class Fake:
        def LocalBundleAdjustment(self, items):
            it = items[0]; n = len(it["obs_kf"])
            er = np.zeros(n, np.uint8); er[[1, 3]] = 1                 # observation 1 is stereo, 3 is monocular
            return [dict(Tcw=np.asarray(it["Tcw"]) + 1, x3Dw=np.asarray(it["x3Dw"]) + 1, erase=er)]

    kfs[3]["covisible"] = [4, 2, 1]; kfs[0] = kf([12, 13]); del kfs[9]
    r = O.LocalBundleAdjustment(Fake(), 3, kfs, mps)
    assert r["erase"] == [(3, 11), (4, 10)]                             # the monocular edges first, then the stereo ones
    O.apply_local_ba(kfs, mps, r)
    assert kfs[4]["mp"][1] == -1 and 4 not in mps[10]["obs"] and kfs[3]["Tcw"][0, 0] == 2.0 and kfs[0]["Tcw"][0, 0] == 1.0 and mps[10]["x3Dw"][2] == 6.0
    assert kfs[3]["mp"][0] == -1 and mps[11]["obs"] == {2: 1, 1: 1} and not mps[11].get("bad")           # two stereo observations are left: four, the point lives
    assert mps[10]["bad"] and mps[10]["obs"] == {} and kfs[3]["mp"][2] == -1 and kfs[2]["mp"][0] == -1   # two monocular ones are left: two, SetBadFlag


def test_a_sanitizer_build_of_the_host_twin_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_local_ba and csrc/host/local_ba.cpp with -fsanitize=address,undefined, run as a program of its own on the scenes of this file"""
    import localba_scene as SC
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "localba_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "sindslam_amd", "csrc"), "sanitize-localba", "OUT=" + exe], check=True, capture_output=True, text=True)
    scenes = [(SC.scene(seed, 3, 1, 30, kind=kind, outliers=4, obs_per_point=3 if seed == 21 else None, id0=seed == 21), 0) for kind in ("mono", "stereo", "mixed") for seed in (2, 21)]
    scenes += [(s, 0) for s in SC.literal_cases().values()] + [(SC.scene(7, 6, 2, 30, kind="mixed", outliers=5), 0)] + [(s, SIND_E_ARG) for s in SC.bad_items().values()]
    with open(tmp_path / "items.bin", "wb") as f:
        f.write(np.ascontiguousarray(SC.K5, np.float32).tobytes()); f.write(np.int32(len(scenes)).tobytes())
        for s, rc in scenes:
            f.write(np.array([len(s["kf_id"]), len(s["mp_id"]), len(s["obs_kf"]), int(s.get("do_more", True)), rc], np.int32).tobytes())
            for k, t in (("kf_id", np.int64), ("kf_kind", np.uint8), ("Tcw", np.float32), ("mp_id", np.int64), ("x3Dw", np.float32), ("obs_start", np.int32), ("obs_kf", np.int32), ("obs_xy", np.float32),
                         ("u_right", np.float32), ("inv_sigma2", np.float32)):
                f.write(np.ascontiguousarray(s[k], t).tobytes())
    r = subprocess.run([exe, str(tmp_path / "items.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(scenes)
    for line, (s, rc) in zip(lines, scenes):                            # and it computed what the library computes
        if rc == 0:
            g = _host(s)
            assert [int(v) for v in line.split()] == [0, g["n_stages"], g["n_level1"], int(g["erase"].sum()), int(np.float64(g["stage_chi2"][1]).view(np.uint64))]
