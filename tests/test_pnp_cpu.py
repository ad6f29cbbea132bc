"""CPU: the host side of PnPsolver (sindh_pnp_pose, sindh_pnp_check, sindh_pnp_refine_plan, sind_pnp_ransac_params; csrc/host/epnp.hpp, csrc/host/pnp.cpp) against the
Python restatement tests/pnp_ref.py, bit for bit; against ground-truth poses, which shares none of the restatement's guesses about OpenCV; and the replay of
Tracking::Relocalization's loop (sindslam_amd/pnp.py) against the literal loop, with the restatement in the device's place."""
import ctypes as C

import numpy as np
import pytest

RELOC = (0.99, 10, 300, 4, 0.5, 5.991)                                  # SetRansacParameters of Tracking::Relocalization


def _same_pose(got, ref, what):
    import pnp_cases as H
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(H.bits64(g), H.bits64(np.array(r, np.float64))), (what, ("R", "t", "error")[k], g, r)


def test_pose_equals_the_restatement_on_samples_of_four_and_on_larger_sets():
    import pnp_cases as H
    import pnp_ref as P
    import pnp_scene as S
    K = H.calib(S.K)
    c = S.candidate(1, 40, outliers=0.3, noise=0.7)
    rng = np.random.default_rng(5)
    for k in range(36):
        s = rng.choice(40, 4, replace=False)
        _same_pose(H.host_pose(c["x3Dw"][s], c["p2d"][s], S.K), P.compute_pose(c["x3Dw"][s], c["p2d"][s], *K), ("sample", k))
    for n in (5, 10, 64):
        for seed, outl in ((n, 0.0), (n + 1, 0.3)):
            d = S.candidate(seed, n, outliers=outl, noise=0.5)
            _same_pose(H.host_pose(d["x3Dw"], d["p2d"], S.K), P.compute_pose(d["x3Dw"], d["p2d"], *K), ("set", n, outl))


def test_pose_equals_the_restatement_on_degenerate_samples():
    """coplanar, collinear, repeated point, a point at the camera centre, one point four times: whatever comes out, NaN included, is the same on both sides"""
    import pnp_cases as H
    import pnp_ref as P
    import pnp_scene as S
    K = H.calib(S.K)
    seen_nan = False
    for name, (X, U) in H.special_samples(S.K).items():
        got = H.host_pose(X, U, S.K)
        _same_pose(got, P.compute_pose(X, U, *K), name)
        seen_nan = seen_nan or bool(np.isnan(got[0]).any())
    assert seen_nan                                                       # found: "all_equal" gives a NaN pose


def test_check_inliers_equals_the_restatement_also_at_zero_depth():
    import pnp_cases as H
    import pnp_ref as P
    import pnp_scene as S
    K = H.calib(S.K)
    for seed, n in ((3, 15), (4, 64), (5, 65), (6, 130)):
        c = S.candidate(seed, n, outliers=0.3, noise=0.8)
        rng = np.random.default_rng(seed)
        for k in range(6):
            s = rng.choice(n, 4, replace=False)
            R, t, _ = H.host_pose(c["x3Dw"][s], c["p2d"][s], S.K)
            if k == 0:                                                    # correspondence 2 at depth exactly 0 under this pose: invZc is infinite, the point no inlier
                c["x3Dw"][2] = H.zero_depth_point(R, t)
                X = [float(v) for v in c["x3Dw"][2]]
                assert R[2][0] * X[0] + R[2][1] * X[1] + R[2][2] * X[2] + t[2] == 0
            cnt, w = H.host_check(c, S.K, R, t)
            inl, rc = P.check_inliers(c["x3Dw"], c["p2d"], c["sigma2"], c["th2"], *K, R.tolist(), t.tolist())
            assert cnt == rc and np.array_equal(w, P.pack_bits(inl)), (seed, k)
            if k == 0:
                assert not inl[2]
        nan = np.full((3, 3), np.nan)
        assert H.host_check(c, S.K, nan, np.zeros(3))[0] == 0 and P.check_inliers(c["x3Dw"], c["p2d"], c["sigma2"], c["th2"], *K, nan.tolist(), [0, 0, 0])[1] == 0


def test_ransac_params_equal_the_restatement():
    import pnp_ref as P
    from sindslam_amd import pnp
    for n in range(4, 401):
        assert pnp.ransac_params(n, *RELOC[:5]) == P.ransac_params(n, *RELOC[:5]), n
        assert pnp.ransac_params(n) == P.ransac_params(n), n
    assert pnp.ransac_params(40, *RELOC[:5]) == (20, 35) and pnp.ransac_params(15, *RELOC[:5]) == (10, 14) and pnp.ransac_params(10, *RELOC[:5]) == (10, 1)


@pytest.mark.parametrize("n", [6, 20, 100])
def test_pose_recovers_the_ground_truth_without_noise(n):
    """Independent of every guess about OpenCV: on exact projections of FP32 map points EPnP must give back the pose.  Measured with the host library over the 50
    seeds below: largest |R - R_true| 1.938e-07 (n = 6), 7.986e-08 (n = 20), 3.367e-08 (n = 100); largest |t - t_true| 1.162e-06, 4.274e-07, 2.189e-07.  The bound of
    a size is ten times its own worst (the margin for other seeds and another build; pnp_cases.BOUNDS); not asserted for n = 4, where the null space of MtM is 4-dimensional."""
    import pnp_cases as H
    import pnp_scene as S
    dR = dt = 0.0
    for seed in range(50):
        c = S.candidate(1000 + seed, n, outliers=0, noise=0)
        R, t, _ = H.host_pose(c["x3Dw"], c["p2d"], S.K)
        dR = max(dR, float(np.abs(R - c["R"]).max())); dt = max(dt, float(np.abs(t - c["t"]).max()))
    print(f"n={n}: largest rotation deviation {dR:.3e}, largest translation deviation {dt:.3e}")
    assert dR <= H.BOUNDS[n][0] and dt <= H.BOUNDS[n][1]


def test_refine_plan_equals_the_restatement():
    import pnp_cases as H
    import pnp_ref as P
    rng = np.random.default_rng(2)
    seqs = [[], [9, 9, 9], [10, 10, 10], [10, 12, 12, 11, 12, 13, 9, 13, 30, 5, 30, 31], [31, 30, 12, 10, 9]] + [list(rng.integers(5, 20, 40)) for _ in range(20)]
    for counts in seqs:
        for best_count, has_best in ((0, False), (12, True), (15, True), (40, True)):
            assert H.host_refine_plan(counts, 10, best_count, has_best) == tuple(P.refine_plan(counts, 10, best_count, has_best)), (counts, best_count)
    # ties refine the unchanged set again, a held set is a problem of its own only when an iteration needs it
    assert H.host_refine_plan([10, 12, 12, 11, 13], 10, 0, False) == ([0, 1, 1, 1, 2], [0, 1, 4])
    assert H.host_refine_plan([10, 12, 13], 10, 12, True) == ([0, 0, 1], [-1, 2]) and H.host_refine_plan([9, 13], 10, 12, True) == ([-1, 0], [1])


def _both_loops(Ns, reject_first, seed=0, outliers=0.3, noise=0.5):
    """the literal loop and the replay on the same candidates and the same random stream, the caller rejecting the first `reject_first` poses (None: every pose)"""
    import pnp_ref as P
    import pnp_scene as S
    from sindslam_amd import pnp
    from sindslam_amd.sim3 import Tape
    cands = [S.candidate(100 + 10 * seed + i, n, outliers=outliers, noise=noise) for i, n in enumerate(Ns)]
    ev = _both_loops.ev
    logs = ([], [])
    def accept(log):
        def f(i, T, vb, n):
            log.append((i, T.tobytes(), tuple(np.flatnonzero(vb)), int(n)))
            return reject_first is not None and len(log) > reject_first
        return f
    drawn = [0]
    rand = S.rand_stream(7 + seed)
    lit = [P.LiteralPnPsolver(ev, c, rand, drawn) for c in cands]
    for s in lit:
        s.SetRansacParameters(*RELOC)
    traces = ([], [])
    ref = P.literal_relocalization(lit, accept(logs[0]), traces[0])
    tape = Tape(S.rand_stream(7 + seed))
    sol = [pnp.PnPsolver(ev, tape, c) for c in cands]
    for s, c in zip(sol, cands):
        s.inp = c; s.SetRansacParameters(*RELOC)                          # the same dict, so that the restatement's cache serves both loops
    calls = ev.calls
    got = pnp.relocalization_pnp(sol, accept(logs[1]), trace=traces[1])
    # every iterate of the loop: which candidate, and its bNoMore; with it the order in which the candidates are discarded
    assert traces[0] == traces[1] and [i for i, no_more in traces[1] if no_more] == ref[4]
    return ref, got, logs, lit, sol, drawn[0], tape.pos, ev.calls - calls, traces[1]


@pytest.fixture(scope="module", autouse=True)
def _evaluator():
    import pnp_ref as P
    import pnp_scene as S
    _both_loops.ev = P.Evaluator(S.K)
    yield
    _both_loops.ev = None


@pytest.mark.parametrize("reject_first", [0, 1, 2, 3, None])
def test_replay_equals_the_literal_loop(reject_first):
    """candidates with N = 9 (fewer than min_inliers: discarded at once), 15, 40, 120"""
    ref, got, logs, lit, sol, drawn, pos, calls, trace = _both_loops([9, 15, 40, 120], reject_first)
    assert logs[0] == logs[1] and len(logs[0]) >= (reject_first or 0)    # every pose offered to the caller: candidate, Tcw, vbInliers, nInliers, in order
    assert got[0] == ref[0] and got[3] == ref[3] and drawn == pos        # the outcome, vbDiscarded, and the reference's position on the tape
    assert [s.mnIterations for s in sol] == [s.mnIterations for s in lit] and [s.mnBestInliers for s in sol] == [s.mnBestInliers for s in lit]
    if got[0] >= 0:
        assert got[1].tobytes() == ref[1].tobytes() and np.array_equal(got[2], ref[2])
    rejected = len(logs[0]) - (got[0] >= 0)
    assert calls <= 1 + rejected                                         # one call, and one more per rejected pose at the most
    assert trace[0] == (0, True)                                         # N = 9 is discarded by its first iterate
    if reject_first is None:
        assert [i for i, no_more in trace if no_more][0] == 0 and sorted(i for i, no_more in trace if no_more) == [0, 1, 2, 3]
        assert got[0] == -1 and all(got[3]) and len(logs[0]) > 5         # found: 11 poses offered, the last of them an exhausted candidate's mBestTcw


def test_replay_where_refine_fails_and_where_a_candidate_exhausts_its_iterations():
    """Refine() tests with `>`: a refined count equal to min_inliers returns nothing.  N = 15 with 5 outliers has at most 10 inliers = min_inliers, so its
    qualifying iterations all call Refine in vain and the candidate ends with bNoMore and mBestTcw.  With 60 % outliers no hypothesis qualifies: no pose at all."""
    import pnp_scene as S
    ref, got, logs, lit, sol, drawn, pos, calls, trace = _both_loops([15, 15], None, seed=4, outliers=5, noise=0.1)
    assert logs[0] == logs[1] and got[3] == ref[3] == [True, True] and drawn == pos and calls == 1
    qualified = [s for s in lit if s.mnBestInliers >= 10]
    assert qualified and all(s.mnBestInliers <= 10 for s in qualified)   # Refine ran and failed: count == min_inliers
    assert len(logs[0]) == len(qualified)                                # each such candidate offers its mBestTcw once, with bNoMore
    assert trace == [(0, True), (1, True)]                               # one iterate each: the or-condition runs it to mRansacMaxIts, then bNoMore
    ref, got, logs, lit, sol, drawn, pos, calls, trace = _both_loops([40, 40, 40], None, seed=3, outliers=0.6)
    assert logs == ([], []) and got[0] == ref[0] == -1 and drawn == pos == 3 * 35 * 4 and calls == 1 and trace == [(0, True), (1, True), (2, True)]


def test_iterate_and_find_on_their_own_equal_the_literal_solver():
    import pnp_ref as P
    import pnp_scene as S
    from sindslam_amd import pnp
    from sindslam_amd.sim3 import Tape
    ev = _both_loops.ev
    for seed, n, outl in ((1, 40, 0.3), (2, 120, 0.5), (3, 9, 0.0)):
        c = S.candidate(300 + seed, n, outliers=outl)
        drawn = [0]
        lit = P.LiteralPnPsolver(ev, c, S.rand_stream(seed), drawn); lit.SetRansacParameters(*RELOC)
        tape = Tape(S.rand_stream(seed)); sol = pnp.PnPsolver(ev, tape, c); sol.inp = c; sol.SetRansacParameters(*RELOC)
        for step in range(6):
            a = lit.iterate(5); b = sol.iterate(5)
            assert (a[0] is None) == (b[0] is None) and a[1] == b[1] and a[3] == b[3] and np.array_equal(np.flatnonzero(a[2]), np.flatnonzero(b[2])) and drawn[0] == tape.pos, (seed, step)
            if a[0] is not None:
                assert a[0].tobytes() == b[0].tobytes() and b[0].dtype == np.float32 and b[0].shape == (4, 4)
            assert len(b[2]) == c["n_keypoints"]
        c2 = S.candidate(400 + seed, n, outliers=outl)
        lit = P.LiteralPnPsolver(ev, c2, S.rand_stream(seed), [0]); tape = Tape(S.rand_stream(seed)); sol = pnp.PnPsolver(ev, tape, c2); sol.inp = c2      # the header's default parameters
        a = lit.iterate(lit.mRansacMaxIts); T, vb, nin = sol.find()
        assert (a[0] is None) == (T is None) and a[3] == nin and np.array_equal(np.flatnonzero(a[2]), np.flatnonzero(vb))


def test_tape_sample_draws_as_the_reference_does():
    import pnp_ref as P
    from sindslam_amd.sim3 import Tape
    rng = np.random.default_rng(0)
    raw = [int(v) for v in rng.integers(0, 2147483648, 400)] + [0, 0, 0, 0, 2147483647, 2147483647, 2147483647, 2147483647]
    tape = Tape(iter(raw).__next__)
    for n in (4, 5, 17, 120):
        for pos in range(0, len(raw) - 4, 4):
            avail = list(range(n)); want = []
            for k in range(4):
                randi = P.random_int(raw[pos + k], 0, len(avail) - 1)
                want.append(avail[randi]); avail[randi] = avail[-1]; avail.pop()
            assert tape.sample(pos, n, 4) == want and len(set(want)) == 4
    assert tape.triple(0, 17) == tape.sample(0, 17, 3)
