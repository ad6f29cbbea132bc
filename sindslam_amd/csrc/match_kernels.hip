// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) on the GPU (reference
// src/ORBmatcher.cc:1328-1470, Frame::GetFeaturesInArea src/Frame.cc:398-451, DescriptorDistance src/ORBmatcher.cc:1647-1665,
// ComputeThreeMaxima :1601-1642).  One workgroup per frame pair, one thread per last-frame map point.
//
// The reference loop is sequential in one respect: a current keypoint that already holds a MapPoint with observations is skipped
// by later points.  Candidate c is therefore closed for point i exactly when some j < i with observations chose c.  The kernel
// solves that recurrence by rounds: every round recomputes all choices against the owners of the previous round
// (minOwner[c] = smallest such j); after round r the first r points are final, and a round without change is the sequential
// result.  Real frames need 2-3 rounds.  The window search keeps the reference's traversal order (cells x-major, push_back order
// inside a cell, strict '<' on the distance), so ties resolve identically.  Integer / bit work: v_bcnt popcounts, L2-resident.
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

#define TH_HIGH 100

struct Proj { float u, v, invzc, radius; int minL, maxL, ok; };

__device__ __forceinline__ Proj d_project(const MatchParams& p, const MatchPose& ps, const float* X, int oct) {
    Proj r; r.ok = 0;
    float xc[3];
    d_to_camera(ps.Tcw, X, xc);
    r.invzc = (float)(1.0 / xc[2]);
    if (r.invzc < 0) return r;
    r.u = p.fx * xc[0] * r.invzc + p.cx; r.v = p.fy * xc[1] * r.invzc + p.cy;
    if (r.u < p.bounds[0] || r.u > p.bounds[1]) return r;
    if (r.v < p.bounds[2] || r.v > p.bounds[3]) return r;
    r.radius = p.th * p.scale[oct];
    if (ps.forward) { r.minL = oct; r.maxL = -1; } else if (ps.backward) { r.minL = 0; r.maxL = oct; } else { r.minL = oct - 1; r.maxL = oct + 1; }
    r.ok = 1; return r;
}

__global__ __launch_bounds__(MT_NT) void k_search_by_projection(MatchParams p, MatchArrays a) {
    __shared__ int changed; __shared__ MatchTailShared tail;
    const int b = blockIdx.x, t = threadIdx.x, nL = min(a.nLast[b], p.capLast), nC = min(a.nCur[b], p.capCur);
    const MatchPose ps = a.pose[b];
    const float* x3Dw = a.x3Dw + (size_t)b * p.capLast * 3; const uint8_t* lflags = a.lastFlags + (size_t)b * p.capLast; const int* loct = a.lastOctave + (size_t)b * p.capLast;
    const float* lang = a.lastAngle + (size_t)b * p.capLast; const uint32_t* ldesc = a.lastDesc + (size_t)b * p.capLast * 8;
    const float* cxy = a.curUnXY + (size_t)b * p.capCur * 2; const int* coct = a.curOctave + (size_t)b * p.capCur; const float* cang = a.curAngle + (size_t)b * p.capCur;
    const float* cur = a.curURight + (size_t)b * p.capCur; const uint32_t* cdesc = a.curDesc + (size_t)b * p.capCur * 8;
    const int* gs = a.gridStart + (size_t)b * 3073; const int* gi = a.gridIdx + (size_t)b * p.capCur; const uint8_t* taken0 = a.curTaken ? a.curTaken + (size_t)b * p.capCur : nullptr;
    int* choice = a.choice + (size_t)b * p.capLast; int* minOwner = a.minOwner + (size_t)b * p.capCur; int* matchOfCur = a.matchOfCur + (size_t)b * p.capCur;
    const float minX = p.bounds[0], minY = p.bounds[2];
    const float wInv = 64.f / (float)(p.bounds[1] - p.bounds[0]), hInv = 48.f / (float)(p.bounds[3] - p.bounds[2]);

    for (int i = t; i < nL; i += MT_NT) choice[i] = -1;
    int round = 0;
    for (;;) {
        for (int c = t; c < nC; c += MT_NT) minOwner[c] = 0x7fffffff;
        if (t == 0) changed = 0;
        __syncthreads();
        for (int i = t; i < nL; i += MT_NT) { const int c = choice[i]; if (c >= 0 && (lflags[i] & 2)) atomicMin(&minOwner[c], i); }
        __syncthreads();
        for (int i = t; i < nL; i += MT_NT) {
            int best = -1;
            if (lflags[i] & 1) {
                const int oct = loct[i];
                const Proj pr = d_project(p, ps, x3Dw + 3 * i, oct);
                if (pr.ok) {
                    const float x = pr.u, y = pr.v, r = pr.radius;
                    const int x0 = max(0, (int)floorf((x - minX - r) * wInv)), x1 = min(63, (int)ceilf((x - minX + r) * wInv));
                    const int y0 = max(0, (int)floorf((y - minY - r) * hInv)), y1 = min(47, (int)ceilf((y - minY + r) * hInv));
                    if (x0 < 64 && x1 >= 0 && y0 < 48 && y1 >= 0) {
                        const bool checkLevels = (pr.minL > 0) || (pr.maxL >= 0);
                        const uint4 d0 = *(const uint4*)(ldesc + 8 * i), d1 = *(const uint4*)(ldesc + 8 * i + 4);
                        const float ur = x - p.bf * pr.invzc;
                        int bestDist = 256;
                        for (int ix = x0; ix <= x1; ix++) {
                            const int jb = gs[ix * 48 + y0], je = gs[ix * 48 + y1 + 1];           // cells (ix, y0..y1) are contiguous in the CSR
                            for (int j = jb; j < je; j++) {
                                const int k = gi[j];
                                if (checkLevels) { const int o = coct[k]; if (o < pr.minL) continue; if (pr.maxL >= 0 && o > pr.maxL) continue; }
                                const float dx = cxy[2 * k] - x, dy = cxy[2 * k + 1] - y;
                                if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
                                if ((taken0 && taken0[k]) || minOwner[k] < i) continue;
                                const float urk = cur[k];
                                if (urk > 0) { const float er = fabsf(ur - urk); if (er > r) continue; }
                                const int dist = d_hamming(cdesc + 8 * k, d0, d1);
                                if (dist < bestDist) { bestDist = dist; best = k; }
                            }
                        }
                        if (bestDist > TH_HIGH) best = -1;
                    }
                }
            }
            if (best != choice[i]) { choice[i] = best; changed = 1; }
        }
        __syncthreads();
        round++;
        const int ch = changed;
        __syncthreads();
        if (!ch || round > nL) break;
    }
    // assignments -> CurrentFrame.mvpMapPoints (the later point wins), rotation histogram, three maxima, removal
    d_assign_and_check_orientation(tail, t, nL, nC, choice, matchOfCur, lang, cang, p.checkOrientation);
    if (t == 0) { a.nmatches[b] = tail.nmatch; a.rounds[b] = round; }
}

int launch_search_by_projection(const MatchParams& p, const MatchArrays& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_search_by_projection, dim3(B), dim3(MT_NT), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
