"""CPU: the host half of Sim3Solver (sindh_sim3_horn, sind_sim3_iterations; sindslam_amd/csrc/host/sim3.cpp) against the Python restatement tests/sim3_ref.py, bit for
bit; against an FP64 SVD solution that shares none of the restatement's guesses about OpenCV; and the replay of LoopClosing::ComputeSim3's loop
(sindslam_amd/sim3.py) against the literal loop, with the restatement's CheckInliers in place of the device."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    """bit patterns, every NaN as one pattern: which NaN an operation returns is the processor's choice among its operands' and decides nothing (no comparison with it holds)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


@pytest.fixture(scope="module")
def host():
    return C.CDLL(os.path.join(ROOT, "sindslam_amd", "libsind_host.so"))


def horn(host, P1, P2, fix):
    P1 = np.ascontiguousarray(P1, np.float32); P2 = np.ascontiguousarray(P2, np.float32)
    R = np.zeros((3, 3), np.float32); t = np.zeros(3, np.float32); s = np.zeros(1, np.float32); T12 = np.zeros((4, 4), np.float32); T21 = np.zeros((4, 4), np.float32)
    host.sindh_sim3_horn(*[C.c_void_p(a.ctypes.data) for a in (P1, P2)], int(fix), *[C.c_void_p(a.ctypes.data) for a in (R, t, s, T12, T21)])
    return dict(R12=R, t12=t, s12=s[0], T12=T12, T21=T21)


def assert_same_bits(got, ref, what):
    for k in ("R12", "t12", "s12", "T12", "T21"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), (what, k, got[k], ref[k])


def random_triples(seed, count, noise=0.01):
    """(P1, P2) 3x3, columns are points: P1 = s R P2 + t, plus noise"""
    import sim3_scene as S
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        R = S.rot(rng.normal(size=3), rng.uniform(0, np.pi)); s = rng.uniform(0.5, 2.0); t = rng.normal(size=3)
        P2 = rng.uniform(-2, 2, (3, 3)) + np.array([[0], [0], [3.0]])
        P1 = s * R @ P2 + t[:, None] + rng.normal(0, noise, (3, 3))
        out.append((P1.astype(np.float32), P2.astype(np.float32), (s, R, t)))
    return out


def test_horn_equals_the_restatement_on_random_triples(host):
    import sim3_ref as R
    for fix in (False, True):
        for k, (P1, P2, _) in enumerate(random_triples(3, 200)):
            assert_same_bits(horn(host, P1, P2, fix), R.compute_sim3(P1, P2, fix), (fix, k))


def test_horn_equals_the_restatement_on_degenerate_and_special_triples(host):
    import sim3_ref as R
    import sim3_scene as S
    p = np.array([0.3, -0.2, 2.0], np.float32)
    same = np.stack([p, p, p], 1)
    line = np.stack([p, p + np.float32(0.5) * np.array([1, 2, 0.5], np.float32), p + np.float32(1.25) * np.array([1, 2, 0.5], np.float32)], 1).astype(np.float32)
    tri = np.array([[0.1, 1.2, -0.7], [0.4, -0.3, 0.9], [2.0, 2.5, 3.1]], np.float32)
    half_turn = (S.rot((0, 0, 1), np.pi) @ tri.astype(np.float64)).astype(np.float32)
    cases = dict(identical=(same, same), collinear=(line, (line * np.float32(1.1)).astype(np.float32)), translation_exact=(tri + np.array([[0.5], [-0.25], [0.125]], np.float32), tri),
                 translation=((tri.astype(np.float64) + np.array([[0.3], [-0.7], [0.1111]])).astype(np.float32), tri),
                 small_turn=((S.rot((1, 2, 3), 1e-3) @ tri.astype(np.float64) + np.array([[0.3], [-0.7], [0.1111]])).astype(np.float32), tri),
                 half_turn=(half_turn, tri), one_side_identical=(tri, same))
    for name, (P1, P2) in cases.items():
        for fix in (False, True):
            got = horn(host, P1, P2, fix)
            assert_same_bits(got, R.compute_sim3(P1, P2, fix), (name, fix))
            if name in ("identical", "translation_exact", "translation"):      # N = 0, or M symmetric up to rounding: Jacobi stops at once (its bound on the pivot is
                #                                                          FLT_EPSILON, absolute), the quaternion is (1, 0, 0, 0) and vec / norm(vec) is 0 * inf.  So the reference's
                #                                                          ComputeSim3 has no answer for a pure translation; a turn of a milliradian is enough for one (below)
                assert np.isnan(got["R12"]).all() and np.isnan(got["t12"]).all() and np.isnan(got["T12"][:3]).all() and np.isnan(got["T21"][:3]).all()
            if name == "small_turn":
                assert np.abs(got["R12"] - S.rot((1, 2, 3), 1e-3)).max() < 1e-5 and np.abs(got["t12"] - [0.3, -0.7, 0.1111]).max() < 1e-5 and abs(got["s12"] - 1) < 1e-5
            if name == "half_turn":
                assert np.abs(got["R12"] - S.rot((0, 0, 1), np.pi)).max() < 1e-5


UMEYAMA_TOL = 4 * 6.75e-5                                                # measured: the largest deviation of an element of R12, t12 or s12 over this test's triples is
#                                                                          6.75e-5 (printed by the test); the margin covers FP32 rounding on other seeds


def umeyama(P1, P2, fix):
    """FP64 SVD solution of P1 = s R P2 + t (Umeyama 1991), points as columns"""
    P1 = P1.astype(np.float64); P2 = P2.astype(np.float64)
    m1 = P1.mean(1, keepdims=True); m2 = P2.mean(1, keepdims=True); A = P1 - m1; B = P2 - m2
    U, D, Vt = np.linalg.svd(A @ B.T)
    S = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    s = 1.0 if fix else np.trace(np.diag(D) @ S) / (B * B).sum()
    return s, R, (m1 - s * R @ m2)[:, 0]


def test_horn_agrees_with_an_fp64_svd_solution_on_noise_free_triples(host, capsys):
    worst = 0.0
    for fix in (False, True):
        for P1, P2, (s, R, t) in random_triples(8, 150, noise=0.0):
            if fix:
                P1 = (R @ P2.astype(np.float64) + t[:, None]).astype(np.float32)
            got = horn(host, P1, P2, fix); us, uR, ut = umeyama(P1, P2, fix)
            dev = max(np.abs(got["R12"] - uR).max(), np.abs(got["t12"] - ut).max(), abs(got["s12"] - us))
            worst = max(worst, dev)
    with capsys.disabled():
        print(f"\nsim3 horn vs FP64 SVD: largest deviation {worst:.3g}")
    assert worst < UMEYAMA_TOL


def test_iterations_equal_the_restatement():
    import sim3_ref as R
    from sindslam_amd.sim3 import ransac_iterations
    for n in (19, 20, 21, 60, 300, 2000):
        assert ransac_iterations(n) == R.ransac_iterations(n), n
    assert ransac_iterations(19) == 0 and ransac_iterations(20) == 1 and ransac_iterations(2000) == 300 and 1 < ransac_iterations(21) < ransac_iterations(60)
    assert ransac_iterations(60, 0.99, 20, 50) == 50 and ransac_iterations(40, 0.5, 10, 300) == R.ransac_iterations(40, 0.5, 10, 300)


def test_random_int_and_the_tape():
    import sim3_ref as R
    from sindslam_amd.sim3 import Tape, random_int
    raw = [0, 1, 2 ** 30, 2 ** 31 - 1, 123456789, 987654321, 5, 2 ** 31 - 2, 77]
    for r in raw:
        for hi in (0, 1, 19, 63, 4095):
            assert random_int(r, 0, hi) == R.random_int(r, 0, hi) and 0 <= random_int(r, 0, hi) <= hi
    assert random_int(32767, 0, 9, rand_max=32767) == 9 and random_int(2 ** 31 - 1, 3, 9) == 9
    taken = []
    def rand():
        taken.append(1); return raw[len(taken) - 1]
    tape = Tape(rand)
    a = tape.triple(0, 20); assert len(taken) == 3                       # lazily
    b = tape.triple(0, 57); assert len(taken) == 3 and a != b            # the same raw values, another N: other indices
    assert tape.triple(3, 20) != a and len(taken) == 6
    for n in (3, 4, 20, 57):                                             # the restatement's draw with the erase-by-swap on a list
        s = R.Solver.__new__(R.Solver); s.N, s.rand, s.rand_max = n, iter(raw).__next__, 2 ** 31 - 1
        t = tape.triple(0, n)
        assert t == s.draw() and len(set(t)) == 3


# ---- the replay ----
def ref_evaluate(requests, fix):
    """the restatement in place of sind_match_sim3_ransac"""
    import sim3_ref as R
    out = []
    for s, tri in requests:
        rs = R.Solver(dict(s.inp), fix, None)
        res = dict(count=[], bits=[], s12=[], R12=[], t12=[])
        for t in tri:
            h = rs.hypothesis(t); inl, cnt = R.check_inliers(rs.sv, h["T12"], h["T21"])
            res["count"].append(cnt); res["bits"].append(R.pack_bits(inl)); res["s12"].append(h["s12"]); res["R12"].append(h["R12"]); res["t12"].append(h["t12"])
        out.append({k: np.array(v) for k, v in res.items()})
    return out


def run_both(inps, raw, script, fix=False, solver_class=None):
    """-> (the literal loop's result, the product's result, candidates per evaluate call); a result is (matched, Scm bits, vbInliers, discarded, log of accept calls);
    script(number of the accept call, candidate) -> accept"""
    import sim3_ref as R
    import sim3_scene as S
    from sindslam_amd.sim3 import Sim3Solver, Tape, compute_sim3
    results, calls = [], []
    for product in (False, True):
        log = []
        def accept(i, Scm, vb):
            ok = script(len(log), i); log.append((i, bits(Scm).copy(), vb.copy(), ok)); return ok
        if not product:
            rand = S.rand_from(raw)
            m, Scm, vb, disc, _ = R.compute_sim3_loop([None if c is None else R.Solver(c, fix, rand) for c in inps], accept)
        else:
            def evaluate(requests, f):
                calls.append(len(requests)); return ref_evaluate(requests, f)
            tape = Tape(S.rand_from(raw))
            solvers = [None if c is None else (solver_class or Sim3Solver)(evaluate, tape, c, fix) for c in inps]
            m, Scm, vb, disc = compute_sim3(solvers, accept)
        results.append((m, None if Scm is None else bits(Scm).copy(), vb, list(disc), log))
    return results[0], results[1], calls


def same_outcome(a, b):
    if a[0] != b[0] or a[3] != b[3] or len(a[4]) != len(b[4]) or (a[1] is None) != (b[1] is None):
        return False
    if a[1] is not None and not (np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])):
        return False
    return all(x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) and x[3] == y[3] for x, y in zip(a[4], b[4]))


@pytest.fixture(scope="module")
def three():
    import sim3_scene as S
    return [S.candidate(1, 60, outliers=0.3)[0], S.candidate(2, 45, outliers=0.25)[0], S.candidate(3, 33, outliers=0.2)[0]]


def test_replay_accepted_first_return(three):
    import sim3_scene as S
    ref, got, calls = run_both(three, S.raw_values(1), lambda k, i: True)
    assert same_outcome(ref, got) and ref[0] >= 0 and len(ref[4]) == 1 and calls == [3]      # one call for all three candidates


def test_replay_rejections_in_every_pattern(three):
    """reject the first r returns, whoever makes them; reject one candidate always; reject everything (every candidate runs out of iterations)"""
    import sim3_scene as S
    for seed in (3, 4):
        raw = S.raw_values(seed)
        for r in (1, 2, 5):
            ref, got, calls = run_both(three, raw, lambda k, i: k >= r)
            assert same_outcome(ref, got) and len(ref[4]) == r + 1 and len(calls) <= r + 1, (seed, r)      # at most one further call per rejection
        first = run_both(three, raw, lambda k, i: True)[0][0]
        ref, got, _ = run_both(three, raw, lambda k, i: i != first)
        assert same_outcome(ref, got) and ref[0] not in (-1, first) and any(x[0] == first and not x[3] for x in ref[4])      # a rejected return, then an accepted one on another candidate
    ref, got, _ = run_both(three, S.raw_values(5), lambda k, i: False)
    assert same_outcome(ref, got) and ref[0] == -1 and ref[3] == [True, True, True] and len(ref[4]) >= 22      # found: 44 returns
    rigid = [S.candidate(21, 50, s12=1.0)[0], S.candidate(22, 40, s12=1.0)[0], S.candidate(23, 30, s12=1.0)[0]]
    ref, got, _ = run_both(rigid, S.raw_values(6), lambda k, i: k >= 1, fix=True)                    # bFixScale, as the RGB-D loop closer sets it
    assert same_outcome(ref, got) and ref[0] >= 0 and len(ref[4]) == 2


def test_replay_without_any_return_and_with_short_and_absent_candidates():
    import sim3_scene as S
    hopeless = [S.candidate(11, 40, outliers=0.8)[0], S.candidate(12, 30, outliers=0.85)[0], S.candidate(13, 24, outliers=0.9)[0]]
    ref, got, calls = run_both(hopeless, S.raw_values(6), lambda k, i: True)
    assert same_outcome(ref, got) and ref[0] == -1 and len(ref[4]) == 0 and ref[3] == [True] * 3 and calls == [3]      # no early return: every candidate runs out of iterations
    mixed = [S.candidate(14, 12, outliers=0.0)[0], None, S.candidate(15, 40, outliers=0.8)[0], S.candidate(16, 50, outliers=0.3)[0]]      # N < 20; discarded on entry; hopeless; good
    ref, got, calls = run_both(mixed, S.raw_values(7), lambda k, i: k >= 1)
    assert same_outcome(ref, got) and ref[0] == 3 and ref[3][:2] == [True, True] and calls[0] == 2


def test_naive_schedule_without_rederivation_gives_another_answer(three):
    """What the re-derivation is for.  Naive: iteration k of candidate i keeps the triple that the schedule drawn before the loop gave it, also after a rejected early
    return.  The reference's next iterate starts where the early return stopped on the tape, so its triples are other ones."""
    import sim3_scene as S
    from sindslam_amd import sim3 as P

    class Naive(P.Sim3Solver):
        first = None

        def iterate(self, nIterations):
            if self.first is None:                                       # the table of the first call, by iteration number
                self.first = [self.table[p] for p in sorted(self.table)]
            for j in range(min(nIterations, self.remaining())):
                self.table[self.tape.pos + 3 * j] = self.first[self.mnIterations + j]
            return super().iterate(nIterations)

    raw = S.raw_values(3)
    script = lambda k, i: k >= 2
    ref, got, _ = run_both(three, raw, script)
    assert same_outcome(ref, got) and len(ref[4]) == 3
    ref2, naive, _ = run_both(three, raw, script, solver_class=Naive)
    assert same_outcome(ref, ref2) and not same_outcome(ref, naive)
    assert ref[4][0][0] == naive[4][0][0] and np.array_equal(ref[4][0][1], naive[4][0][1])      # up to the first rejection the two are the same
