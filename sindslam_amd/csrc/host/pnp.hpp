// Host half of PnPsolver (reference src/PnPsolver.cc) around epnp.hpp: SetRansacParameters, the list of Refine problems of a candidate, and the
// test entries of libsind_host.so.  Plain C++: compiled into libsind_hip.so (capi_match_ransac.cpp calls it) and into libsind_host.so.
#pragma once
#include <cstdint>

namespace sind {

// The Refine() problems of one candidate over its evaluated iterations (PnPsolver::iterate :209-236).  Refine is a pure function of mvbBestInliers, and that set
// changes only on a strict `>` of an iteration with count >= minInliers; every other qualifying iteration refines the unchanged set again.  So the distinct problems
// are the strict prefix maxima of count that are >= minInliers, in iteration order, continuing from the bestCount the solver holds; the set it holds (hasBest)
// is a problem of its own (hypothesis row -1) if a qualifying iteration comes before the first new maximum.
//   refineOfHyp [nIts]: index into the list of the problem iteration h refines, -1 if count[h] < minInliers (-2: it would need the held set, and hasBest is false)
//   hypOfRefine [nIts + 1]: the iteration whose inlier set problem r is, -1 for the held set.  -> the number of problems
int pnp_refine_plan(const int* count, int nIts, int minInliers, int bestCount, bool hasBest, int* refineOfHyp, int* hypOfRefine);

}  // namespace sind
