"""CPU: the host twin of sind_match_global_ba (sindh_global_ba, csrc/host/global_ba.hpp) against the Python restatement tests/globalba_ref.py bit for bit; against the
parent's sindh_local_ba (stage 1) on all-stereo scenes; the envelope factor against the dense definition; the reduced-system path against numpy's solve of the full
system; the literal cases, the error paths and every limit through the plan alone; the Python tails of sindslam_amd/optimizer.py on a toy map; and a sanitizer build of
the host twin run as its own process."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

SCHUR_DEVIATION = 1.06e-13                                               # profiles/match_local_ba.txt: |x - numpy's solve of the full (6P + 3M) system| / |x|; the arithmetic is the same here
LBA_C = 56
SIND_E_ARG, SIND_E_CAPACITY = -1, -5
NO_ENV = ("Tcw", "x3Dw", "included", "n_iters", "chi2", "lambda_", "n_active_poses", "solver_fail")


def _host(s, iterations=10, robust=False):
    import globalba_scene as G
    return G.HostGBA().GlobalBundleAdjustment([s], iterations, robust)[0]


def _ref(s, iterations=10, robust=False):
    import globalba_ref as R
    import globalba_scene as G
    return R.global_ba(s, G.K5, iterations, robust)


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("robust", [0, 1])
def test_host_library_equals_the_restatement_bit_for_bit(kind, robust):
    """5 key frames x 24 points, 3 of a window of 4 key frames per point, 4 planted outliers: with kernels the monocular ones exercise the sqrt(5.99) delta"""
    import globalba_scene as G
    s = G.band_map({"mono": 2, "stereo": 21, "mixed": 22}[kind], 5, 24, 4, 3, kind=kind, outliers=4)
    for iterations in (0, 1, 10, 20):
        g = _host(s, iterations, robust)
        G.assert_same(g, _ref(s, iterations, robust), (kind, robust, iterations), keys=NO_ENV)
        assert (g["n_iters"] > 0) == (iterations > 0) and g["n_active_poses"] == 4
    if robust and kind == "mono":                                       # the delta is this function's: local BA's sqrt(5.991) gives other bits on the same item
        import globalba_ref as R
        keep = R.DELTA
        R.DELTA = {False: R.F(R.f32(np.sqrt(R.F(5.991)))), True: keep[True]}
        try:
            other = _ref(s, 10, 1)
        finally:
            R.DELTA = keep
        assert other["chi2"] != _host(s, 10, 1)["chi2"]


def _local_twin(s):
    import localba_scene as SC
    return SC.HostBA().LocalBundleAdjustment([dict(s, do_more=False)])[0]


def test_the_parent_as_yardstick():
    """all-stereo scenes with key frames of kinds 0 and 1 only: sindh_global_ba(iterations = 5, robust = 1) is sindh_local_ba(do_more = 0), stage 1 of the parent's call, bit
    for bit: the same arithmetic in the same orders, the envelope factor in place of the dense one.  With and without key frame 0, with a point that has no observation
    and with a free key frame that has no edge."""
    import globalba_scene as G
    import localba_scene as SC
    scenes = [SC.scene(41, 5, 0, 40, kind="stereo", outliers=4, obs_per_point=3, id0=True), SC.scene(42, 4, 0, 40, kind="stereo", outliers=4, obs_per_point=None),
              SC.scene(43, 8, 0, 60, kind="stereo", outliers=5, obs_per_point=2, id0=True)]
    scenes.append(G.without_point_obs(scenes[0], 7))
    scenes.append(G.without_kf_obs(scenes[0], 3))
    assert scenes[4]["kf_kind"][3] == 0
    for n, s in enumerate(scenes):
        it, order = G.from_local(s)
        loc = _local_twin(s); g = _host(it, 5, True)
        assert np.array_equal(SC.bits(g["Tcw"]), SC.bits(loc["Tcw"][order])) and np.array_equal(SC.bits(g["x3Dw"]), SC.bits(loc["x3Dw"])), n
        assert g["n_iters"] == loc["stage_iters"][0] and SC.bits(np.float64(g["chi2"])) == SC.bits(np.float64(loc["stage_chi2"][0])) and SC.bits(np.float64(g["lambda_"])) == SC.bits(np.float64(loc["stage_lambda"][0])), n
    assert _host(G.from_local(scenes[3])[0], 5, True)["included"][7] == 0


def _mixed_window():
    """a local window of 3 free key frames (index 2 without an edge), the fixed key frame with id 0 (index 3) and a fixed camera (index 4) whose observations are all
    monocular; 38 points seen by three key frames each, one point seen by the two fixed cameras alone and one seen by key frame 0 alone -> the scene"""
    import globalba_scene as G
    import localba_scene as SC
    s = SC.scene(61, 3, 2, 38, kind="mixed", outliers=3, obs_per_point=3)
    s["kf_kind"] = np.array([0, 0, 0, 1, 2], np.uint8); s["kf_id"] = s["kf_id"].copy(); s["kf_id"][3] = 0
    s = G.without_kf_obs(s, 2)
    s["u_right"] = np.where(s["obs_kf"] == 4, np.float32(-1.0), s["u_right"]).astype(np.float32)
    X = np.array([0.3, -0.2, 6.0]); Y = np.array([-0.6, 0.4, 5.2])
    s = SC.with_point(s, X + 0.02, [SC.seen(s, 3, X, mono=False), SC.seen(s, 4, X)])
    return SC.with_point(s, Y - 0.02, [SC.seen(s, 3, Y, mono=False)])


def _observations(s, keep):
    """a copy of the scene with the observations of the mask alone"""
    out = dict(s)
    for key in ("obs_kf", "obs_xy", "u_right", "inv_sigma2", "planted"):
        out[key] = s[key][keep]
    out["obs_start"] = np.concatenate([[0], np.cumsum(keep)])[np.asarray(s["obs_start"])].astype(np.int32)
    return out


def _as_global(s):
    """the scene as a global-BA item: the key frames in ascending kf_id (globalba_scene.from_local, which refuses fixed cameras) -> item, order"""
    order = np.argsort(s["kf_id"], kind="stable"); inv = np.empty(len(order), np.int32); inv[order] = np.arange(len(order), dtype=np.int32)
    it = {k: s[k] for k in ("mp_id", "x3Dw", "obs_start", "obs_xy", "u_right", "inv_sigma2")}
    it.update(kf_id=np.asarray(s["kf_id"])[order], Tcw=np.asarray(s["Tcw"])[order], obs_kf=inv[np.asarray(s["obs_kf"], np.int64)])
    return it, order


def _global_linear(it, robust):
    import globalba_scene as G
    from sindslam_amd.matcher import globalba_items
    arr, keep = globalba_items([it])
    P = int((np.asarray(it["kf_id"]) != 0).sum())
    Cc = np.zeros((len(it["obs_kf"]), LBA_C)); x = np.zeros(6 * P + 3 * len(it["mp_id"])); lam = np.zeros(1)
    K = np.ascontiguousarray(G.K5)
    assert G.host().sindh_globalba_linear(C.addressof(arr), robust, K.ctypes.data, Cc.ctypes.data, x.ctypes.data, lam.ctypes.data) == 0
    return Cc, x, lam[0]


def test_both_bundle_adjustments_linearise_and_solve_a_mixed_window_alike():
    """The phases the two bundle adjustments share (csrc/host/ba_schur.hpp) through both views, beyond the all-stereo case: the first linearisation and the first
    trial's solve of a mixed mono / stereo window with 3 free and 2 fixed key frames, 40 points, a point seen by fixed cameras alone and a free key frame without an
    edge.  C, x and lambda bit for bit, (1) sindh_globalba_linear(robust = 1) against sindh_localba_linear on the stereo observations alone, where the Huber deltas of
    the two agree, and (2) sindh_globalba_linear(robust = 0) against the numpy restatement on the whole window.
    Global BA fixes the key frame with id 0 and no other.  The window's second fixed camera therefore carries monocular observations only: among the stereo
    observations it has none, so global BA holds it as one more free key frame without an edge (no Hessian index, its six entries of x stay +0), and (1) compares
    the same reduced system.  In (2) it is a free pose of global BA and of its restatement, and the point that only key frame 0 sees is the one seen by fixed cameras
    alone."""
    import globalba_ref as GR
    import globalba_scene as G
    import localba_scene as SC
    from sindslam_amd.matcher import localba_items
    s = _mixed_window()
    assert list(s["kf_kind"]) == [0, 0, 0, 1, 2] and len(s["mp_id"]) == 40 and not (s["obs_kf"] == 2).any()
    assert (s["u_right"] < 0).any() and (s["u_right"] >= 0).any() and (s["u_right"][s["obs_kf"] == 4] < 0).all()
    assert set(s["obs_kf"][s["obs_start"][38]:s["obs_start"][39]]) == {3, 4} and list(s["obs_kf"][s["obs_start"][39]:]) == [3]
    # (1) the stereo observations alone, through both views
    st = _observations(s, s["u_right"] >= 0)
    assert len(st["obs_kf"]) > 40 and not (st["obs_kf"] == 4).any()
    arr, keep = localba_items([st])
    n_obs, M = len(st["obs_kf"]), 40
    Cl = np.zeros((n_obs, LBA_C)); xl = np.zeros(6 * 3 + 3 * M); ll = np.zeros(1)
    K = np.ascontiguousarray(SC.K5)
    SC.host().sindh_localba_linear.argtypes = [C.c_void_p] * 5
    assert SC.host().sindh_localba_linear(C.addressof(arr), K.ctypes.data, Cl.ctypes.data, xl.ctypes.data, ll.ctypes.data) == 0
    it, order = _as_global(st)
    Cg, xg, lg = _global_linear(it, 1)
    free_g = [k for k in order if int(st["kf_id"][k]) != 0]              # global BA's pose ranks as key frames of the scene
    free_l = sorted([k for k in range(5) if st["kf_kind"][k] == 0], key=lambda k: int(st["kf_id"][k]))
    assert len(free_g) == 4 and [k for k in free_g if k != 4] == free_l
    poses = np.concatenate([xg[6 * free_g.index(k):6 * free_g.index(k) + 6] for k in free_l])
    assert np.array_equal(SC.bits(Cg), SC.bits(Cl)) and SC.bits(np.float64(lg)) == SC.bits(np.float64(ll[0])) and lg > 0
    assert np.array_equal(SC.bits(poses), SC.bits(xl[:18])) and np.array_equal(SC.bits(xg[24:]), SC.bits(xl[18:]))
    assert not SC.bits(xg[6 * free_g.index(4):6 * free_g.index(4) + 6]).any() and not SC.bits(xl[6 * free_l.index(2):6 * free_l.index(2) + 6]).any() and np.abs(xl).max() > 1e-4
    # (2) the whole window without kernels against the restatement
    it, order = _as_global(s)
    Cg, xg, lg = _global_linear(it, 0)
    with np.errstate(all="ignore"):
        g = GR.Graph(it, G.K5)
        assert g.activate() > 0 and g.n_act == 3 and g.P == 4
        g.x = [GR.ZERO] * (6 * g.P + 3 * g.n_mp)
        g.evaluate(False, True); g.sums()
        lam = GR.F(1e-5) * g.max_diagonal()
        Cr = np.zeros_like(Cg)
        for e, c in enumerate(g.C):
            if "Hp" in c:
                Cr[e, 0:21] = c["Hp"]; Cr[e, 21:27] = c["bp"]; Cr[e, 36:54] = np.array(c["Hpl"]).reshape(18)
            Cr[e, 27:33] = c["Hl"]; Cr[e, 33:36] = c["bl"]; Cr[e, 54] = c["rho0"]; Cr[e, 55] = c["chi2"]
        assert g.solve(lam)
    assert np.array_equal(SC.bits(Cg), SC.bits(Cr)) and SC.bits(np.float64(lg)) == SC.bits(np.float64(lam)) and np.array_equal(SC.bits(xg), SC.bits(np.array(g.x, np.float64)))
    assert sum("Hp" not in c for c in g.C) >= 3 and np.abs(xg[6 * g.P + 3 * 39:]).max() > 0


def test_envelope_with_a_loop_equals_the_dense_restatement():
    """40 key frames, window 5, one loop (2, 37): block row 37 starts at block column 2, the rows between do not; the restatement factors the dense 234 x 234"""
    import globalba_scene as G
    s = G.band_map(31, 40, 60, 5, 3, loops=((2, 37),), kind="mixed", outliers=3)
    g = _host(s, 1, True)
    assert g["env_entries"] < g["env_dense_entries"] == 36 * 39 * 40 // 2 and g["n_active_poses"] == 39
    G.assert_same(g, _ref(s, 1, True), "loop", keys=NO_ENV)


def _dense_ldlt(H, b):
    """the dense definition of csrc/host/local_ba.hpp with NumPy FP64 scalars -> x, D"""
    n = len(b); L = [[np.float64(0.0)] * n for _ in range(n)]; D = [np.float64(0.0)] * n
    for j in range(n):
        for i in range(j, n):
            v = np.float64(H[j][i])
            for k in range(j):
                v = v - (L[i][k] * D[k]) * L[j][k]
            if i == j:
                D[j] = v
            else:
                L[i][j] = v / D[j]
    y = [np.float64(v) for v in b]
    for j in range(n):
        for i in range(j + 1, n):
            y[i] = y[i] - L[i][j] * y[j]
    y = [y[i] / D[i] for i in range(n)]
    for j in range(n - 1, 0, -1):
        for i in range(j):
            y[i] = y[i] - L[j][i] * y[j]
    return np.array(y), np.array(D)


def test_envelope_factor_alone_against_the_dense_definition_and_the_zero_pivot():
    """the three factor phases and the solves on a given matrix: an empty, a short and a full envelope row; a zero pivot fails and leaves x untouched (in a whole call
    lambda > 0 stands on every diagonal entry whenever any is non-zero, so this rule is reached through the factor's own entry point)"""
    import globalba_scene as G
    h = G.host(); h.sindh_globalba_factor.argtypes = [C.c_int] + [C.c_void_p] * 5
    rng = np.random.RandomState(5)
    first = np.array([0, 0, 2, 1, 4, 0, 5], np.int32); nb = len(first); n = 6 * nb
    A = np.zeros((n, n))
    for I in range(nb):
        for J in range(first[I], I + 1):
            A[6 * I:6 * I + 6, 6 * J:6 * J + 6] = rng.normal(0, 1, (6, 6))
    H = np.tril(A) + np.tril(A, -1).T + 12 * np.eye(n); b = rng.normal(0, 1, n)
    x = np.full(n, 7.0); D = np.zeros(n)
    assert h.sindh_globalba_factor(nb, first.ctypes.data, np.ascontiguousarray(H).ctypes.data, b.ctypes.data, x.ctypes.data, D.ctypes.data) == 0
    with np.errstate(all="ignore"):
        xr, Dr = _dense_ldlt(H, b)
    assert np.array_equal(x.view(np.uint64), xr.view(np.uint64)) and np.array_equal(D.view(np.uint64), Dr.view(np.uint64))
    assert np.linalg.norm(x - np.linalg.solve(H, b)) <= 1e-12 * np.linalg.norm(x)
    H0 = H.copy(); H0[0, :] = 0.0; H0[:, 0] = 0.0                                                   # D(0) = 0
    x = np.full(n, 7.0)
    assert h.sindh_globalba_factor(nb, first.ctypes.data, np.ascontiguousarray(H0).ctypes.data, b.ctypes.data, x.ctypes.data, D.ctypes.data) == 1
    assert (x == 7.0).all() and D[0] == 0.0


def _full_system(s, Cc, lam):
    """the full (6P + 3M) system of the first linearisation from the edges' contributions, lambda on the diagonal -> H, b"""
    free = [k for k in range(len(s["kf_id"])) if int(s["kf_id"][k]) != 0]
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
    """the first linearisation of the four scene sizes of the local-BA test (5 key frames of which 4 free, 30 points, every key frame or 3 per point): x of the Schur
    complement, the envelope LDL^T and the back-substitution against numpy's solve of the whole system, at the tolerance that test records"""
    import globalba_scene as G
    from sindslam_amd.matcher import globalba_items
    worst = 0.0
    for seed, kind in ((31, "mono"), (32, "stereo"), (33, "mixed"), (34, "mixed")):
        s = G.band_map(seed, 5, 30, 5, 5 if seed < 34 else 3, kind=kind, outliers=3)
        arr, keep = globalba_items([s])
        n_obs, P, M = len(s["obs_kf"]), 4, len(s["mp_id"])
        Cc = np.zeros((n_obs, LBA_C)); x = np.zeros(6 * P + 3 * M); lam = np.zeros(1)
        K = np.ascontiguousarray(G.K5)
        assert G.host().sindh_globalba_linear(C.addressof(arr), 1, K.ctypes.data, Cc.ctypes.data, x.ctypes.data, lam.ctypes.data) == 0
        H, b = _full_system(s, Cc, lam[0])
        ref = np.linalg.solve(H, b)
        dev = np.linalg.norm(x - ref) / np.linalg.norm(ref)
        print(f"seed {seed} {kind}: relative deviation {dev:.3e}")
        worst = max(worst, dev)
        assert lam[0] > 0 and np.linalg.norm(ref) > 1e-3
    print(f"Schur path against numpy's solve of the full system: largest relative deviation {worst:.3e}")
    assert worst <= 4 * SCHUR_DEVIATION


def test_literal_and_degenerate_cases():
    import globalba_scene as G
    import localba_scene as SC
    import poseopt_ref as PR
    rt = lambda T: PR.to_tcw(PR.from_tcw(T))
    # only key frame 0: no active pose, the points alone move (the empty factorisation succeeds)
    s = G.band_map(12, 1, 9, 1, 1, kind="stereo"); g = _host(s, 10, True)
    G.assert_same(g, _ref(s, 10, True), "P0", keys=NO_ENV)
    assert g["n_active_poses"] == 0 and g["n_iters"] > 0 and g["env_entries"] == 0 and np.array_equal(SC.bits(g["Tcw"][0]), SC.bits(rt(s["Tcw"][0]))) and g["x3Dw"].tobytes() != s["x3Dw"].tobytes()
    # no observations at all, and no points: nothing is optimised, the outputs are the conversions alone
    base = G.band_map(11, 4, 14, 4, 3, kind="mixed")
    none = dict(base, obs_start=np.zeros(len(base["mp_id"]) + 1, np.int32), obs_kf=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32), u_right=np.zeros(0, np.float32), inv_sigma2=np.zeros(0, np.float32))
    nomp = dict(none, mp_id=np.zeros(0, np.int64), x3Dw=np.zeros((0, 3), np.float32), obs_start=np.zeros(1, np.int32))
    for name, it in (("n_obs0", none), ("n_mp0", nomp)):
        g = _host(it, 10, False)
        G.assert_same(g, _ref(it, 10, False), name, keys=NO_ENV)
        assert (g["n_iters"], g["chi2"], g["lambda_"], g["n_active_poses"], g["solver_fail"]) == (-1, 0.0, -1.0, 0, 0) and not g["included"].any()
        assert g["x3Dw"].tobytes() == it["x3Dw"].tobytes() and all(np.array_equal(SC.bits(g["Tcw"][k]), SC.bits(rt(it["Tcw"][k]))) for k in range(4))
    assert G.HostGBA().GlobalBundleAdjustment([]) == []                   # B = 0
    # iterations = 0: the stop flag set at entry
    g = _host(base, 0, True)
    assert g["n_iters"] == 0 and g["lambda_"] == -1.0 and g["x3Dw"].tobytes() == base["x3Dw"].tobytes() and g["included"].all()
    # no fixed key frame: every pose has a Hessian index
    s = G.band_map(13, 4, 14, 4, 3, kind="mixed", first_id=3); g = _host(s, 10, False)
    G.assert_same(g, _ref(s, 10, False), "no fixed", keys=NO_ENV)
    assert g["n_active_poses"] == 4 and g["Tcw"][0].tobytes() != rt(s["Tcw"][0]).tobytes()
    # a point without observations keeps its input and is reported; a free key frame without an edge keeps the round trip of its pose
    s = G.without_kf_obs(G.without_point_obs(base, 3), 2); g = _host(s, 10, False)
    G.assert_same(g, _ref(s, 10, False), "holes", keys=NO_ENV)
    assert g["included"][3] == 0 and g["included"].sum() == 13 and g["x3Dw"][3].tobytes() == s["x3Dw"][3].tobytes() and g["n_active_poses"] == 2
    assert np.array_equal(SC.bits(g["Tcw"][2]), SC.bits(rt(s["Tcw"][2]))) and g["Tcw"][1].tobytes() != rt(s["Tcw"][1]).tobytes()
    # a rejected last trial: a point at depth 0 in the fixed key frame (the identity) has an infinite chi2, rho is NaN, the one trial of every iteration is rejected
    # (NaN fails the stop criteria too, so all ten iterations run): the estimates are the popped ones, the round trip of the input
    z0 = dict(base); z0["Tcw"] = base["Tcw"].copy(); z0["Tcw"][0] = np.eye(4, dtype=np.float32)
    X = np.array([0.3, -0.2, 6.0])
    s = SC.with_point(z0, [0.5, 0.25, 0.0], [(0, 300.0, 200.0, -1.0, 1.0), SC.seen(base, 1, X), SC.seen(base, 2, X)]); g = _host(s, 10, False)
    G.assert_same(g, _ref(s, 10, False), "depth0", keys=NO_ENV)
    assert np.isinf(g["chi2"]) and g["n_iters"] == 10 and g["x3Dw"].tobytes() == s["x3Dw"].tobytes() and all(np.array_equal(SC.bits(g["Tcw"][k]), SC.bits(rt(s["Tcw"][k]))) for k in range(4))


def _plan(it):
    import globalba_scene as G
    from sindslam_amd.matcher import globalba_items
    arr, keep = globalba_items([it])
    sizes = np.zeros(4)
    return G.host().sindh_globalba_plan(C.addressof(arr), sizes.ctypes.data), sizes


def _bare(n_kf, obs_lists):
    """an item of n_kf key frames (ids 1 ..) and one point per list of key-frame indices, without geometry: the plan reads counts and indices alone"""
    n_mp = len(obs_lists); obs_kf = np.concatenate(obs_lists).astype(np.int32) if n_mp else np.zeros(0, np.int32)
    start = np.concatenate([[0], np.cumsum([len(o) for o in obs_lists])]).astype(np.int32)
    T = np.tile(np.eye(4, dtype=np.float32), (n_kf, 1, 1))
    return dict(kf_id=np.arange(1, n_kf + 1, dtype=np.int64), Tcw=T, mp_id=np.arange(n_mp, dtype=np.int64), x3Dw=np.ones((n_mp, 3), np.float32), obs_start=start, obs_kf=obs_kf,
                obs_xy=np.zeros((len(obs_kf), 2), np.float32), u_right=np.zeros(len(obs_kf), np.float32), inv_sigma2=np.ones(len(obs_kf), np.float32))


def test_every_capacity_limit_through_the_plan_alone():
    """4096 key frames, 2^20 points, 2^22 observations, 2^26 co-observation entries, 2^25 stored entries of the envelope: at the limit the plan succeeds (where that is
    cheap), one beyond it is SIND_E_CAPACITY, decided from the counts before any list is built"""
    assert _plan(_bare(4096, [[0, 1]]))[0] == 0 and _plan(_bare(4097, [[0, 1]]))[0] == SIND_E_CAPACITY
    empty = np.zeros(0, np.int32)
    assert _plan(_bare(2, [empty] * (1 << 20)))[0] == 0 and _plan(_bare(2, [empty] * ((1 << 20) + 1)))[0] == SIND_E_CAPACITY
    lists = [np.arange(8, dtype=np.int32)] * (1 << 19)                    # 2^22 observations (2^19 * 36 co-observation entries, a dense 8 x 8 envelope) and one more
    assert _plan(_bare(8, lists + [np.array([0], np.int32)]))[0] == SIND_E_CAPACITY
    # the envelope: one point seen by every one of n key frames makes it the dense triangle, 36 n (n + 1) / 2 entries: n = 1364 is the last that fits 2^25
    n = 1365
    assert 36 * n * (n + 1) // 2 > (1 << 25) >= 36 * (n - 1) * n // 2
    assert _plan(_bare(n, [np.arange(n, dtype=np.int32)]))[0] == SIND_E_CAPACITY
    rc, sizes = _plan(_bare(n - 1, [np.arange(n - 1, dtype=np.int32)]))
    assert rc == 0 and sizes[2] == 36 * (n - 1) * n // 2 and sizes[1] == (n - 1) * n // 2
    rc, sizes = _plan(_bare(n, [[0, n - 1]] + [[k, k + 1] for k in range(n - 1)]))     # a chain and one loop: rows 1 .. n - 2 hold two blocks, the last row is full
    assert rc == 0 and sizes[2] == 36 * (1 + 2 * (n - 2) + n)
    # the co-observation lists: points seen by 181 consecutive key frames each (181 * 182 / 2 = 16 471 entries a point), a band whose envelope stays below its own
    # limit (36 * 181 * 4096 < 2^25): 4 075 such points are 67 119 325 > 2^26 entries, 4 074 are not
    per = 181 * 182 // 2
    need = (1 << 26) // per + 1
    assert 36 * 181 * 4096 < (1 << 25) and need * per > (1 << 26) >= (need - 1) * per
    band = [np.arange(k % 3900, k % 3900 + 181, dtype=np.int32) for k in range(need)]
    assert _plan(_bare(4096, band))[0] == SIND_E_CAPACITY and _plan(_bare(4096, band[:40]))[0] == 0


def test_error_paths_write_nothing():
    import globalba_scene as G
    from sindslam_amd.matcher import globalba_items
    good = G.band_map(601, 4, 8, 4, 3, kind="mixed")
    K = np.ascontiguousarray(G.K5)
    for name, bad in G.bad_items().items():
        arr, keep = globalba_items([good, bad])
        for a in keep:
            a["Tcw_out"][:] = 7.0; a["x3Dw_out"][:] = 7.0; a["included"][:] = 7; a["n_iters"][:] = 7
        assert G.host().sindh_global_ba(arr, 2, 10, 0, K.ctypes.data) == SIND_E_ARG, name
        for a in keep:
            assert (a["Tcw_out"] == 7.0).all() and (a["x3Dw_out"] == 7.0).all() and (a["included"] == 7).all() and a["n_iters"][0] == 7, name
    arr, keep = globalba_items([good])
    h = G.host()
    assert h.sindh_global_ba(None, 1, 10, 0, K.ctypes.data) == SIND_E_ARG and h.sindh_global_ba(arr, -1, 10, 0, K.ctypes.data) == SIND_E_ARG
    assert h.sindh_global_ba(arr, 1, -1, 0, K.ctypes.data) == SIND_E_ARG and h.sindh_global_ba(arr, 1, 10, 0, None) == SIND_E_ARG
    arr, keep = globalba_items([good]); arr[0].included = None
    assert h.sindh_global_ba(arr, 1, 10, 0, K.ctypes.data) == SIND_E_ARG
    for field in ("n_kf", "n_mp"):                                        # a negative count
        arr, keep = globalba_items([good]); setattr(arr[0], field, -1)
        assert h.sindh_global_ba(arr, 1, 10, 0, K.ctypes.data) == SIND_E_ARG
    for field in ("Tcw", "x3Dw", "obs_kf", "Tcw_out"):                    # a NULL array with a non-zero count
        arr, keep = globalba_items([good]); setattr(arr[0], field, None)
        assert h.sindh_global_ba(arr, 1, 10, 0, K.ctypes.data) == SIND_E_ARG
    arr, keep = globalba_items([good, G.band_map(602, 4097, 2, 2, 2, kind="mono")])
    keep[0]["Tcw_out"][:] = 7.0
    assert h.sindh_global_ba(arr, 2, 10, 0, K.ctypes.data) == SIND_E_CAPACITY and (keep[0]["Tcw_out"] == 7.0).all()


def _toy(seed=3):
    """localba_scene.toy_map with a spanning tree (a chain), reference key frames and the fields of the global-BA tail"""
    import localba_scene as SC
    kfs, mps, _ = SC.toy_map(seed, n_kf=5, n_pts=60, outliers=0.0)
    for k in kfs:
        kfs[k]["parent"] = k - 1 if k else None; kfs[k]["children"] = {k + 1} if k + 1 in kfs else set()
    for m in mps:
        mps[m]["ref_kf"] = min(mps[m]["obs"])
    return kfs, mps


def test_apply_global_ba():
    import copy

    import globalba_scene as G
    from sindslam_amd import optimizer as O
    kfs, mps = _toy()
    mps[7]["obs"] = {}                                                    # a point the graph does not include
    res = O.GlobalBundleAdjustment(G.HostGBA(), kfs, mps, 10, False)
    item = res["item"]; r = res["result"]
    assert list(item["kfs"]) == sorted(kfs) and list(item["mps"]) == sorted(mps) and 7 not in res["points"] and r["included"].sum() == len(mps) - 1
    e0 = int(item["obs_start"][item["mps"].index(5)])                     # the observations of a point in ascending key-frame id
    ks = sorted(mps[5]["obs"])
    assert [item["kfs"][i] for i in item["obs_kf"][e0:e0 + len(ks)]] == ks and np.array_equal(item["obs_xy"][e0], kfs[ks[0]]["un_xy"][mps[5]["obs"][ks[0]]])
    A, B = (copy.deepcopy(kfs), copy.deepcopy(mps)), (copy.deepcopy(kfs), copy.deepcopy(mps))
    O.apply_global_ba(A[0], A[1], res, 0)
    O.apply_global_ba(B[0], B[1], res, 9)
    for i, k in enumerate(item["kfs"]):
        assert A[0][k]["Tcw"].tobytes() == r["Tcw"][i].tobytes() and "TcwGBA" not in A[0][k]
        assert B[0][k]["TcwGBA"].tobytes() == r["Tcw"][i].tobytes() and B[0][k]["ba_global_for_kf"] == 9 and np.array_equal(B[0][k]["Tcw"], kfs[k]["Tcw"])
    for j, m in enumerate(item["mps"]):
        if m == 7:
            assert A[1][m]["x3Dw"].tobytes() == mps[m]["x3Dw"].tobytes() and "PosGBA" not in B[1][m]
        else:
            assert A[1][m]["x3Dw"].tobytes() == r["x3Dw"][j].tobytes() and B[1][m]["PosGBA"].tobytes() == r["x3Dw"][j].tobytes() and B[1][m]["ba_global_for_kf"] == 9
            assert B[1][m]["x3Dw"].tobytes() == mps[m]["x3Dw"].tobytes()


def test_run_global_bundle_adjustment_against_the_literal_loop():
    """a toy map; while the BA runs, local mapping adds two key frames (children of 4 and of the first new one) and three points (referenced to key frames 4, 5 and 6):
    the tail moves them through the spanning tree, written out here literally with numpy's FP32 scalars"""
    import copy

    import globalba_scene as G
    from sindslam_amd import optimizer as O
    kfs, mps = _toy()
    f = np.float32

    def during(K, M):
        for k in (5, 6):
            D = np.eye(4, dtype=np.float32); D[0, 3] = 0.1 * (k - 4); D[2, 3] = -0.05
            K[k] = dict(Tcw=(D @ K[4]["Tcw"]).astype(np.float32), parent=k - 1, children=set(), bad=False)
            K[k - 1]["children"].add(k)
        for n, (m, ref) in enumerate(((900, 4), (901, 5), (902, 6))):
            M[m] = dict(x3Dw=np.array([0.1 * n, -0.2, 5.5 + n], np.float32), obs={}, bad=False, ref_kf=ref)

    K0, M0 = copy.deepcopy(kfs), copy.deepcopy(mps)
    during(K0, M0)
    trace = {}
    r = O.run_global_bundle_adjustment(G.HostGBA(), kfs, mps, 4, [0], during=during, trace=trace)
    item = trace["item"]
    assert r["n_iters"] >= 2 and len(item["kfs"]) == 5 and 5 in kfs and 902 in mps

    def mul(A, B):
        return np.array([[((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j] for j in range(4)] for i in range(4)], np.float32)

    def inv(T):
        W = np.eye(4, dtype=np.float32); W[:3, :3] = T[:3, :3].T; W[:3, 3] = -(T[:3, :3].T @ T[:3, 3]); return W

    def cam(T, X):
        return np.array([((T[i, 0] * X[0] + T[i, 1] * X[1]) + T[i, 2] * X[2]) + T[i, 3] for i in range(3)], np.float32)

    gba = {k: np.array(r["Tcw"][i], np.float32) for i, k in enumerate(item["kfs"])}
    assert f(1) * gba[4][0, 0] == gba[4][0, 0]
    gba[5] = mul(mul(K0[5]["Tcw"], inv(K0[4]["Tcw"])), gba[4])            # Tchildc = Tcw_child * Twc; mTcwGBA = Tchildc * parent.mTcwGBA
    gba[6] = mul(mul(K0[6]["Tcw"], inv(K0[5]["Tcw"])), gba[5])            # the parent's pose is still the uncorrected one when its children are visited
    for k in range(7):
        assert kfs[k]["Tcw"].tobytes() == gba[k].tobytes() and kfs[k]["TcwBefGBA"].tobytes() == K0[k]["Tcw"].tobytes() and kfs[k]["ba_global_for_kf"] == 4, k
    for j, m in enumerate(item["mps"]):
        assert mps[m]["x3Dw"].tobytes() == np.asarray(r["x3Dw"][j], np.float32).tobytes()
    for m, ref in ((900, 4), (901, 5), (902, 6)):
        want = cam(inv(gba[ref]), cam(K0[ref]["Tcw"], M0[m]["x3Dw"]))
        assert mps[m]["x3Dw"].tobytes() == want.tobytes() and mps[m]["x3Dw"].tobytes() != M0[m]["x3Dw"].tobytes(), m
    # nLoopKF == 0 (the call outside loop closing): SetPose and SetWorldPos, no tail
    kfs2, mps2 = _toy()
    r2 = O.run_global_bundle_adjustment(G.HostGBA(), kfs2, mps2, 0, [0])
    assert all(kfs2[k]["Tcw"].tobytes() == r2["Tcw"][k].tobytes() and "TcwBefGBA" not in kfs2[k] for k in kfs2)


def test_a_sanitizer_build_of_the_host_twin_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_global_ba and csrc/host/global_ba.cpp with -fsanitize=address,undefined, run as a program of its own on the scenes of this file"""
    import globalba_scene as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "globalba_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "sindslam_amd", "csrc"), "sanitize-globalba", "OUT=" + exe], check=True, capture_output=True, text=True)
    base = G.band_map(11, 4, 14, 4, 3, kind="mixed")
    none = dict(base, obs_start=np.zeros(len(base["mp_id"]) + 1, np.int32), obs_kf=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2), np.float32), u_right=np.zeros(0, np.float32), inv_sigma2=np.zeros(0, np.float32))
    nomp = dict(none, mp_id=np.zeros(0, np.int64), x3Dw=np.zeros((0, 3), np.float32), obs_start=np.zeros(1, np.int32))
    scenes = [(G.band_map(seed, 5, 24, 4, 3, kind=kind, outliers=4), it, rb, 0) for kind, seed in (("mono", 2), ("stereo", 21), ("mixed", 22)) for it, rb in ((10, 1), (20, 0), (0, 1))]
    scenes += [(G.band_map(31, 40, 60, 5, 3, loops=((2, 37),), kind="mixed", outliers=3), 3, 1, 0), (G.band_map(12, 1, 9, 1, 1, kind="stereo"), 10, 1, 0), (none, 10, 0, 0), (nomp, 10, 0, 0),
               (G.band_map(13, 4, 14, 4, 3, kind="mixed", first_id=3), 10, 0, 0), (G.without_kf_obs(G.without_point_obs(base, 3), 2), 10, 0, 0)]
    scenes += [(s, 10, 0, SIND_E_ARG) for s in G.bad_items().values()]
    with open(tmp_path / "items.bin", "wb") as f:
        f.write(np.ascontiguousarray(G.K5, np.float32).tobytes()); f.write(np.int32(len(scenes)).tobytes())
        for s, it, rb, rc in scenes:
            f.write(np.array([len(s["kf_id"]), len(s["mp_id"]), len(s["obs_kf"]), it, rb, rc], np.int32).tobytes())
            for k, t in (("kf_id", np.int64), ("Tcw", np.float32), ("mp_id", np.int64), ("x3Dw", np.float32), ("obs_start", np.int32), ("obs_kf", np.int32), ("obs_xy", np.float32),
                         ("u_right", np.float32), ("inv_sigma2", np.float32)):
                f.write(np.ascontiguousarray(s[k], t).tobytes())
    r = subprocess.run([exe, str(tmp_path / "items.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(scenes)
    for line, (s, it, rb, rc) in zip(lines, scenes):                    # and it computed what the library computes
        if rc == 0:
            g = _host(s, it, rb)
            assert [int(v) for v in line.split()] == [0, g["n_iters"], g["n_active_poses"], int(g["included"].sum()), g["env_entries"], int(np.float64(g["chi2"]).view(np.uint64)),
                                                     int(np.asarray(g["Tcw"], np.float32).reshape(-1)[11:12].view(np.uint32)[0])]
