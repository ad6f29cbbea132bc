"""Sim3Solver and the RANSAC loop of LoopClosing::ComputeSim3 (reference src/Sim3Solver.cc, src/LoopClosing.cc:282-342) over sind_match_sim3_ransac.

The reference draws three indices per iteration from rand() and tests the hypothesis at once.  The sample of an iteration depends only on the random stream
and on N, never on an earlier result, so here the raw values go on a Tape, the triples of every iteration that can still run are drawn from it ahead of time, one
call evaluates them all (ComputeSim3 on the host, CheckInliers on the device), and Sim3Solver.iterate replays the reference's bookkeeping over the table of
counts.  compute_sim3 does this for all candidates of a loop closure with one call.  When an iterate returns early and the caller rejects its Scm, the later
calls of the reference consume the stream in another interleaving (the early return ended that call's batch of 5): the schedule that remains is then drawn
again from the same tape, from the position the reference has reached, and evaluated with one further call per rejection.  The result equals the reference's
loop for any sequence of rejections.  The only difference is on the random stream: raw values are consumed beyond the point where the reference would have
stopped (Tape.pos is the reference's position, len(Tape.raw) what was taken from `rand`)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib

RAND_MAX = 2147483647                                                   # glibc's


def random_int(raw, lo, hi, rand_max=RAND_MAX):
    """DUtils::Random::RandomInt(lo, hi) (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) on a raw rand() value"""
    d = hi - lo + 1
    return int((float(raw) / (float(rand_max) + 1.0)) * d) + lo


def ransac_iterations(n, probability=0.99, min_inliers=20, max_its=300):
    """mRansacMaxIts after SetRansacParameters (:114-138); 0 if n < min_inliers (sind_sim3_iterations)"""
    f = lib().sind_sim3_iterations; f.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int]
    return int(f(int(n), float(probability), int(min_inliers), int(max_its)))


class Tape:
    """The values of rand() in the order the reference's process would get them, filled lazily from `rand` (a callable that returns the next raw value).  The same
    raw value yields another index when another candidate consumes it, because RandomInt scales it by that candidate's N: so the tape holds raw values, not indices."""

    def __init__(self, rand, rand_max=RAND_MAX):
        self.rand, self.rand_max, self.raw, self.pos = rand, rand_max, [], 0

    def at(self, k):
        while len(self.raw) <= k:
            self.raw.append(int(self.rand()))
        return self.raw[k]

    def triple(self, pos, n):
        """the idx of :166-177 for the three draws at tape positions pos .. pos + 2 among n correspondences"""
        moved, out = {}, []
        for i in range(3):
            size = n - i
            randi = random_int(self.at(pos + i), 0, size - 1, self.rand_max)
            out.append(moved.get(randi, randi))
            moved[randi] = moved.get(size - 1, size - 1)                  # vAvailableIndices[randi] = vAvailableIndices.back(); pop_back()
        return out

    def sample(self, pos, n, k):
        """the k distinct idx that k draws at tape positions pos .. pos + k - 1 take from vAvailableIndices = 0 .. n - 1 (PnPsolver::iterate :188-201, k = mRansacMinSet)"""
        moved, out = {}, []
        for i in range(k):
            size = n - i
            randi = random_int(self.at(pos + i), 0, size - 1, self.rand_max)
            out.append(moved.get(randi, randi))
            moved[randi] = moved.get(size - 1, size - 1)
        return out


class Sim3Solver:
    """Sim3Solver of the reference, its state and semantics; made by ORBmatcher.sim3_solvers.  iterate / find / GetEstimated* as there; SetRansacParameters as there."""

    def __init__(self, evaluate, tape, inp, fix_scale):
        """evaluate(requests, fix_scale): requests = [(solver, triples [k, 3])] -> [dict(count [k], bits [k, words], s12 [k], R12 [k, 3, 3], t12 [k, 3])];
        inp: T1w, T2w, x3Dw1, x3Dw2, sigma2_1, sigma2_2 per correspondence, indices1 = mvnIndices1, N1 = mN1"""
        self.evaluate, self.tape, self.inp, self.fix_scale = evaluate, tape, inp, bool(fix_scale)
        self.mN1 = int(inp["N1"]); self.mvnIndices1 = np.asarray(inp["indices1"], np.int64); self.N = len(self.mvnIndices1)
        self.mnBestInliers = 0
        self.mBestT12 = self.mBestRotation = self.mBestTranslation = self.mBestScale = self.mvbBestInliers = None
        self.table = {}                                                  # tape position of an iteration's first draw -> its evaluated hypothesis
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=20, maxIterations=300):
        self.mRansacMinInliers = minInliers
        self.mRansacMaxIts = ransac_iterations(self.N, probability, minInliers, maxIterations)      # 0: iterate leaves at :146
        self.mnIterations = 0

    def remaining(self):
        return max(0, self.mRansacMaxIts - self.mnIterations)

    def request(self, positions):
        """the triples of the iterations that would start at these tape positions"""
        return self, np.array([self.tape.triple(p, self.N) for p in positions], np.int32).reshape(-1, 3)

    def store(self, positions, res):
        for k, p in enumerate(positions):
            self.table[p] = {key: res[key][k] for key in ("count", "bits", "s12", "R12", "t12")}

    def iterate(self, nIterations):
        """-> (Scm [4, 4] float32 or None, bNoMore, vbInliers bool [mN1], nInliers)"""
        vbInliers = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vbInliers, 0
        k = min(nIterations, self.remaining())
        need = [self.tape.pos + 3 * j for j in range(k)]
        if any(p not in self.table for p in need):                       # on its own (find, or iterate outside compute_sim3): one call for this call's iterations
            self.store(need, self.evaluate([self.request(need)], self.fix_scale)[0])
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts and nCurrentIterations < nIterations:
            nCurrentIterations += 1; self.mnIterations += 1
            h = self.table[self.tape.pos]; self.tape.pos += 3
            if h["count"] >= self.mnBestInliers:
                inl = ((h["bits"][np.arange(self.N) >> 6] >> (np.arange(self.N) & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
                T12 = np.eye(4, dtype=np.float32); T12[:3, :3] = np.float32(h["s12"]) * h["R12"] + np.float32(0); T12[:3, 3] = h["t12"]
                self.mvbBestInliers, self.mnBestInliers, self.mBestT12 = inl, int(h["count"]), T12
                self.mBestRotation, self.mBestTranslation, self.mBestScale = h["R12"].copy(), h["t12"].copy(), np.float32(h["s12"])
                if h["count"] > self.mRansacMinInliers:
                    vbInliers[self.mvnIndices1[inl]] = True
                    return self.mBestT12, False, vbInliers, int(h["count"])
        return None, self.mnIterations >= self.mRansacMaxIts, vbInliers, 0

    def find(self):
        """-> (Scm or None, vbInliers12, nInliers)"""
        Scm, _, vb, n = self.iterate(self.mRansacMaxIts)
        return Scm, vb, n

    def GetEstimatedRotation(self):
        return self.mBestRotation.copy()

    def GetEstimatedTranslation(self):
        return self.mBestTranslation.copy()

    def GetEstimatedScale(self):
        return self.mBestScale


def _plan(solvers, discarded, tape, first):
    """The reference's order of iterations from its present state (the for loop is about to reach candidate `first`) if no iterate returned early from here on
    -> per solver, the tape positions of its iterations"""
    left = [0 if d else s.remaining() for s, d in zip(solvers, discarded)]
    plan, pos = [[] for _ in solvers], tape.pos
    while any(left):
        for i in range(first, len(solvers)):
            for _ in range(min(5, left[i])):
                plan[i].append(pos); pos += 3
            left[i] -= min(5, left[i])
        first = 0
    return plan


def compute_sim3(solvers, accept, batch=None):
    """The `while(nCandidates>0 && !bMatch)` loop of LoopClosing::ComputeSim3 (:286-342).  solvers: one Sim3Solver per initial candidate on one Tape, None where
    vbDiscarded[i] is set on entry (bad key frame, fewer than 20 matches).  accept(i, Scm, vbInliers) is the caller's SearchBySim3 + OptimizeSim3 and returns whether
    nInliers >= 20.  All hypotheses are evaluated by one sind_match_sim3_ransac call (`batch` candidates per call if there are more than the handle's max_batch), and
    by one further call after every rejected Scm.  -> (index of the matched candidate or -1, Scm or None, vbInliers or None, vbDiscarded)"""
    discarded = [s is None for s in solvers]
    live = [s for s in solvers if s is not None]
    nCandidates = len(live)
    if not live:
        return -1, None, None, discarded
    tape, evaluate, fix = live[0].tape, live[0].evaluate, live[0].fix_scale
    assert all(s.tape is tape for s in live)

    def fill(first):
        plan = _plan(solvers, discarded, tape, first)
        todo = [(solvers[i], p) for i, p in enumerate(plan) if p]
        if all(q in s.table for s, p in todo for q in p):                # an early return at the end of its batch of 5 shifts nothing
            return
        step = batch or len(todo) or 1
        for a in range(0, len(todo), step):
            for (s, p), res in zip(todo[a:a + step], evaluate([s.request(p) for s, p in todo[a:a + step]], fix)):
                s.store(p, res)

    fill(0)
    while nCandidates > 0:
        for i, s in enumerate(solvers):
            if discarded[i]:
                continue
            Scm, bNoMore, vbInliers, nInliers = s.iterate(5)
            if bNoMore:
                discarded[i] = True; nCandidates -= 1
            if Scm is not None:
                if accept(i, Scm, vbInliers):
                    return i, Scm, vbInliers, discarded
                fill(i + 1)                                                # the early return shifted every later iteration on the tape
    return -1, None, None, discarded
