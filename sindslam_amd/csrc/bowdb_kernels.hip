// KeyFrameDatabase's scoring on the GPU (reference src/KeyFrameDatabase.cc:76-309 up to the list and graph logic, which stays with the caller):
// one query BowVector against the BowVector of every stored key frame.
//   common      the number of words both vectors hold = mnLoopWords / mnRelocWords (a key frame sits once in the inverted list of each of its words, :86-104)
//   firstWord   the smallest common word: the word at whose list the reference first meets the key frame, which with the order of `add` gives the order of
//               lKFsSharingWords
//   score       L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): sum over the common words, ascending, of fabs(vi - wi) - fabs(vi) - fabs(wi)
//               in FP64, left to right, vi the query's value; then (float)(-sum / 2.0), the float the reference stores in mLoopScore / mRelocScore
// One wave per (query, slot).  The query's words sit 64 at a time in the lanes, every lane finds its word in the slot's ascending words by bisection and
// forms its term; a ballot gives the count, and the terms are added one after another in ascending lane order through v_readlane over the ballot's bits:
// a tree reduction would round differently, and score >= minScore decides a loop candidate (:136).  -ffp-contract=off keeps the term's three operations apart.
#include "match.hpp"

namespace sind {

#define DB_NT 256

__device__ __forceinline__ double d_lane_f64(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

__global__ __launch_bounds__(DB_NT) void k_bowdb_query(BowDbArrays a, int capSlots, int capWords) {
    const int q = blockIdx.y, lane = threadIdx.x & 63, slot = __builtin_amdgcn_readfirstlane(blockIdx.x * (DB_NT / 64) + (threadIdx.x >> 6));
    if (slot >= capSlots) return;
    const size_t out = (size_t)q * capSlots + slot;
    const int ns = min(a.slotN[slot], capWords), nq = min(a.qN[q], capWords);
    if (ns < 0) { if (lane == 0) { a.common[out] = 0; a.firstWord[out] = -1; a.score[out] = 0.0f; } return; }      // a dead slot
    const int* sw = a.slotWord + (size_t)slot * capWords; const double* sv = a.slotValue + (size_t)slot * capWords;
    const int* qw = a.qWord + (size_t)q * capWords; const double* qv = a.qValue + (size_t)q * capWords;
    int common = 0, first = -1; double sum = 0.0;
    for (int c0 = 0; c0 < nq; c0 += 64) {
        const int i = c0 + lane; int word = 0; bool hit = false; double term = 0.0;
        if (i < nq) {
            word = qw[i];
            int lo = 0, hi = ns;                                   // lower_bound
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (sw[mid] < word) lo = mid + 1; else hi = mid; }
            if (lo < ns && sw[lo] == word) { hit = true; const double vi = qv[i], wi = sv[lo]; term = fabs(vi - wi) - fabs(vi) - fabs(wi); }
        }
        unsigned long long m = __ballot(hit);
        if (!m) continue;
        if (first < 0) first = __builtin_amdgcn_readlane(word, __builtin_ctzll(m));
        common += __popcll(m);
        for (; m; m &= m - 1) sum = sum + d_lane_f64(term, __builtin_ctzll(m));
    }
    if (lane == 0) { a.common[out] = common; a.firstWord[out] = first; a.score[out] = (float)(-sum / 2.0); }
}

int launch_bowdb_query(const BowDbArrays& a, int capSlots, int capWords, int Q, hipStream_t s) {
    hipLaunchKernelGGL(k_bowdb_query, dim3(divup(capSlots, DB_NT / 64), Q), dim3(DB_NT), 0, s, a, capSlots, capWords);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
