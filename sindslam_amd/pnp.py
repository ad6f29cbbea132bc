"""PnPsolver and the RANSAC loop of Tracking::Relocalization (reference src/PnPsolver.cc, src/Tracking.cc:1435-1533) over sind_match_pnp_ransac.

The reference draws four indices per iteration from rand() and solves and tests the hypothesis at once.  The sample of an iteration depends only on the random
stream and on N, never on an earlier result, so here the raw values go on a sim3.Tape, the samples of every iteration that can still run are drawn from it ahead
of time, one call evaluates them all on the device (EPnP, CheckInliers, and the Refine problems that follow from the counts), and PnPsolver.iterate replays the
reference's bookkeeping over the table.  The loop condition of iterate is `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`, an OR: the
iterate(5, ...) of Relocalization runs until mRansacMaxIts is reached, and at least 5 iterations, unless a Refine returns early.  So, if nobody returned early,
every candidate would run max(mRansacMaxIts - mnIterations, 5) iterations in its turn and be discarded: that is the schedule drawn ahead.  When an iterate returns a
pose early and the caller rejects it, the later calls read the tape from an earlier position than planned: the schedule that remains is drawn again from the
position the reference has reached, and evaluated with one further call per rejection.  The result equals the reference's loop for any sequence of rejections.
The only difference is on the random stream: raw values are consumed beyond the point where the reference would have stopped (Tape.pos is the reference's
position, len(Tape.raw) what was taken from `rand`)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib


def ransac_params(n, probability=0.99, min_inliers=8, max_its=300, min_set=4, epsilon=0.4):
    """(mRansacMinInliers, mRansacMaxIts) after SetRansacParameters (:121-157) for n correspondences (sind_pnp_ransac_params)"""
    f = lib().sind_pnp_ransac_params; f.restype = None
    f.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    a, b = C.c_int(), C.c_int()
    f(int(n), float(probability), int(min_inliers), int(max_its), int(min_set), float(epsilon), C.byref(a), C.byref(b))
    return a.value, b.value


def _unpack(bits, n):
    i = np.arange(n)
    return ((bits[i >> 6] >> (i & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def _tcw(R, t):
    """mBestTcw / mRefinedTcw: the FP64 R, t converted to FP32 (convertTo), in an identity"""
    T = np.eye(4, dtype=np.float32); T[:3, :3] = np.asarray(R, np.float64).astype(np.float32); T[:3, 3] = np.asarray(t, np.float64).astype(np.float32)
    return T


class PnPsolver:
    """PnPsolver of the reference, its state and semantics; made by ORBmatcher.pnp_solvers.  SetRansacParameters, iterate and find as there."""

    def __init__(self, evaluate, tape, inp):
        """evaluate(requests): requests = [(inp, samples [k, 4], min_inliers, best_count, best_bits or None)] -> what ORBmatcher.PnPRansac returns;
        inp: x3Dw, p2d, sigma2 per correspondence, indices = mvKeyPointIndices, n_keypoints = mvpMapPointMatches.size()"""
        self.evaluate, self.tape = evaluate, tape
        self.inp = dict(inp)
        self.mvKeyPointIndices = np.asarray(inp["indices"], np.int64); self.N = len(self.mvKeyPointIndices); self.nKeypoints = int(inp["n_keypoints"])
        self.mnIterations = 0; self.mnBestInliers = 0; self.mvbBestInliers = None; self.mBestTcw = None
        self.mnRefinedInliers = 0; self.mvbRefinedInliers = None; self.mRefinedTcw = None
        self.max_batch = None                                            # of the handle, set by ORBmatcher.pnp_solvers
        self.table, self.table_next = {}, None                           # tape position of an iteration's first draw -> its evaluated hypothesis and what Refine() gives there
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        self.mRansacMinInliers, self.mRansacMaxIts = ransac_params(self.N, probability, minInliers, maxIterations, minSet, epsilon) if self.N else (max(minInliers, minSet), 1)
        self.mRansacMinSet = minSet
        self.inp["th2"] = float(np.float32(th2))
        self.table, self.table_next = {}, None

    def planned(self, nIterations=5):
        """how many iterations the next iterate(nIterations) runs if no Refine returns early"""
        if self.N < self.mRansacMinInliers:
            return 0
        return max(self.mRansacMaxIts - self.mnIterations, nIterations)

    def request(self, positions):
        """the evaluation of the iterations that would start at these tape positions, from the best set the solver holds now"""
        samples = np.array([self.tape.sample(p, self.N, self.mRansacMinSet) for p in positions], np.int32).reshape(-1, 4)
        bits = None
        if self.mvbBestInliers is not None:
            bits = np.zeros((self.N + 63) // 64, np.uint64)
            for i in np.flatnonzero(self.mvbBestInliers):
                bits[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
        return self.inp, samples, self.mRansacMinInliers, self.mnBestInliers, bits

    def store(self, positions, res):
        self.table = {}                                                  # an evaluation holds for the best set it started from: nothing older is kept
        self.table_next = positions[0] if len(positions) else None       # and for this solver's iterations taken in this order: Refine's set follows the counts before it
        for k, p in enumerate(positions):
            r = int(res["refine"][k])
            self.table[p] = dict(count=int(res["count"][k]), bits=res["bits"][k], R=res["R"][k], t=res["t"][k],
                                 refine=None if r < 0 else {key: res["refine_" + key][r] for key in ("count", "bits", "R", "t")})

    def _out(self, inl):
        vb = np.zeros(self.nKeypoints, bool); vb[self.mvKeyPointIndices[inl]] = True
        return vb

    def iterate(self, nIterations):
        """-> (Tcw [4, 4] float32 or None, bNoMore, vbInliers bool over all keypoints (all false where the reference leaves the vector empty), nInliers)"""
        none = np.zeros(self.nKeypoints, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, none, 0
        assert self.mRansacMinSet == 4, "sind_match_pnp_ransac evaluates samples of four"
        need = [self.tape.pos + 4 * j for j in range(self.planned(nIterations))]
        if self.tape.pos != self.table_next or any(p not in self.table for p in need):                       # on its own (find, or iterate outside relocalization_pnp): one call for this call's iterations
            assert len(need) <= 300, "one sind_match_pnp_ransac call evaluates at most 300 iterations of a candidate"
            self.store(need, self.evaluate([self.request(need)])[0])
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts or nCurrentIterations < nIterations:
            nCurrentIterations += 1; self.mnIterations += 1
            h = self.table[self.tape.pos]; self.tape.pos += 4; self.table_next = self.tape.pos
            if h["count"] >= self.mRansacMinInliers:
                if h["count"] > self.mnBestInliers:
                    self.mvbBestInliers, self.mnBestInliers, self.mBestTcw = _unpack(h["bits"], self.N), h["count"], _tcw(h["R"], h["t"])
                r = h["refine"]                                          # Refine() on mvbBestInliers
                self.mnRefinedInliers, self.mvbRefinedInliers = int(r["count"]), _unpack(r["bits"], self.N)
                if self.mnRefinedInliers > self.mRansacMinInliers:
                    self.mRefinedTcw = _tcw(r["R"], r["t"])
                    return self.mRefinedTcw.copy(), False, self._out(self.mvbRefinedInliers), self.mnRefinedInliers
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                return self.mBestTcw.copy(), True, self._out(self.mvbBestInliers), self.mnBestInliers
            return None, True, none, 0
        return None, False, none, 0

    def find(self):
        """-> (Tcw or None, vbInliers, nInliers)"""
        Tcw, _, vb, n = self.iterate(self.mRansacMaxIts)
        return Tcw, vb, n


def _plan(solvers, discarded, tape, first):
    """The reference's order of iterations from its present state (the for loop is about to reach candidate `first`) if no iterate returned a pose early from here
    on: every live candidate runs max(mRansacMaxIts - mnIterations, 5) iterations in its turn and reports bNoMore -> per solver, the tape positions of its iterations"""
    plan, pos = [[] for _ in solvers], tape.pos
    for i in list(range(first, len(solvers))) + list(range(first)):
        if discarded[i]:
            continue
        for _ in range(solvers[i].planned(5)):
            plan[i].append(pos); pos += 4
    return plan


def relocalization_pnp(solvers, accept, batch=None, trace=None):
    """The `while(nCandidates>0 && !bMatch)` loop of Tracking::Relocalization (src/Tracking.cc:1435-1527).  solvers: one PnPsolver per candidate key frame on one Tape,
    None where vbDiscarded[i] is set on entry.  accept(i, Tcw, vbInliers, nInliers) is the caller's PoseOptimization / SearchByProjection chain (:1460-1524) and returns
    whether nGood >= 50.  All hypotheses are evaluated by one sind_match_pnp_ransac call (`batch` candidates per call if there are more than the handle's max_batch),
    and by one further call after every rejected pose.  batch None: the handle's max_batch where ORBmatcher.pnp_solvers made the solvers.  trace: a list that gets
    (i, bNoMore) of every iterate in order, so also the order in which candidates are discarded.  -> (index of the matched candidate or -1, Tcw or None, vbInliers or None, vbDiscarded)"""
    discarded = [s is None for s in solvers]
    live = [s for s in solvers if s is not None]
    nCandidates = len(live)
    if not live:
        return -1, None, None, discarded
    tape, evaluate = live[0].tape, live[0].evaluate
    assert all(s.tape is tape for s in live)
    batch = batch or getattr(live[0], "max_batch", None)

    def fill(first):
        plan = _plan(solvers, discarded, tape, first)
        todo = [(solvers[i], p) for i, p in enumerate(plan) if p]
        step = batch or len(todo) or 1
        for a in range(0, len(todo), step):
            for (s, p), res in zip(todo[a:a + step], evaluate([s.request(p) for s, p in todo[a:a + step]])):
                s.store(p, res)

    fill(0)
    while nCandidates > 0:
        for i, s in enumerate(solvers):
            if discarded[i]:
                continue
            Tcw, bNoMore, vbInliers, nInliers = s.iterate(5)
            if trace is not None:
                trace.append((i, bool(bNoMore)))
            if bNoMore:
                discarded[i] = True; nCandidates -= 1
            if Tcw is not None:
                if accept(i, Tcw, vbInliers, nInliers):
                    return i, Tcw, vbInliers, discarded
                if not bNoMore:
                    fill(i + 1)                                            # the early return shifted every later iteration on the tape, and this solver's best set may have changed
    return -1, None, None, discarded
