// The two vocabulary-guided searches on the GPU:
//   ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches)   reference src/ORBmatcher.cc:159-288   (TrackReferenceKeyFrame, Relocalization)
//   ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)   :657-823, CheckDistEpipolarLine :140-157   (LocalMapping::CreateNewMapPoints)
//   ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12)   :522-655   (LoopClosing::ComputeSim3, once per loop candidate)
// All walk two DBoW2 feature vectors node by node and compare only keypoints that share a node.  A keypoint has one node, and DBoW2 fills a node's index list in
// keypoint order (FeatureVector.cpp:31-45), so the per-keypoint node id the vocabulary transform returns (bow_kernels.hip) carries the whole map: nodes are
// independent of one another, and inside a node the entries act in ascending keypoint index.  Side A is the side whose entries act (pKF / pKF1), side B the side
// searched (F / pKF2).  Three launches per call, B pairs each:
//   k_bow_group   one workgroup per (pair, side): (node, index) keys sorted in LDS (bitonic, 8 B per key, at most BOW_MAX_KEYS), node -1 (not in the feature
//                 vector) last; the first entry of every node of side A is listed.  No host loop touches a keypoint.
//   k_bow_match / k_tri_match   one wave per (pair, node of side A): side B's range of that node is found by a 64-ary search over the lanes; its keypoints
//                 sit in the lanes, in chunks of 64 when there are more (the first chunk's data stays in registers, later chunks are read again per
//                 entry); side A's entries are loaded 64 at a time, one per lane, then taken one after another through v_readlane, and every one ends
//                 in a wave-wide minimum -- so no global load sits on the path from one entry to the next.
//     SearchByBoW: the one sequential dependence -- an entry skips frame keypoints an earlier entry of the node claimed (:209) -- is kept by that order; the claims
//       are one bit per chunk in a lane's register.  best = min over (distance, position) = the first of the smallest, as the strict '<' scan finds it;
//       bestDist2 = the minimum again without that position = the second element of the sorted distances, equal ones included.  TH_LOW 50 with '<=', then the
//       ratio test in FP32.
//     SearchByBoW(pKF1, pKF2) is k_bow_match<true>: side A is pKF1, side B pKF2; side B carries validity too (!pMP2 || isBad() is skipped like a claimed
//       keypoint, :576-580, so it starts as a claim), the claims are vbMatched2, and the bound is 'bestDist1 < TH_LOW', strict (:598).  The result is
//       vpMatches12 by idx1 and so is the rotation histogram (both angles mvKeysUn): the tail is k_tri_tail.
//     SearchForTriangulation: vbMatched2 is never set in the reference, so the entries are independent: among the node's idx2 that pass the tests (no map
//       point, the stereo flags, dist <= 50, the epipole distance for mono-mono pairs, the epipolar line) the smallest distance, the later one on equal distance
//       ('dist > bestDist' is the skip test) = min over (distance, -position).
//   k_bow_tail / k_tri_tail   one workgroup per pair: rotation histogram, ComputeThreeMaxima, removal (match_device.hpp); the triangulation tail is indexed by
//                 idx1, since several idx1 may share an idx2.
// Measured once, profiles/match_bow.txt.
// Arithmetic of the triangulation tests (FP32 left to right unless said; -ffp-contract=off, IEEE division):
//   C2 = R2w * Cw + t2w          d_to_camera's product; invz = 1.0f / C2z; ex = fx * C2x * invz + cx, ey likewise
//   a, b, c                      x1 * F12(0,j) + y1 * F12(1,j) + F12(2,j);  num = a * x2 + b * y2 + c;  den = a * a + b * b, den == 0 rejects;  dsqr = num * num / den
//   (double)dsqr < 3.84 * (double)mvLevelSigma2[octave2], mvLevelSigma2[l] = scale[l] * scale[l] in FP32
//   epipole: distex * distex + distey * distey < 100 * scale[octave2] rejects
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

#define TH_LOW 50
#define BW_NT 256
#ifndef BW_GROUPS
#define BW_GROUPS 32                                               // workgroups per pair: 128 waves share a pair's nodes (1 / 8 / 32 measured, profiles/match_bow.txt)
#endif

__global__ __launch_bounds__(MT_NT) void k_bow_group(BowParams p, BowArrays a, int B) {
    extern __shared__ unsigned long long keys[];                   // node << 32 | index; sortLen of them
    __shared__ int nseg, nvalid;
    const int b = blockIdx.x, side = blockIdx.y, t = threadIdx.x, cap = side ? p.capB : p.capA;
    const int n = min(min(side ? a.nB[b] : a.nA[b], cap), p.sortLen);
    const int* node = (side ? a.nodeB : a.nodeA) + (size_t)b * cap;
    int2* sorted = (side ? a.sortedB : a.sortedA) + (size_t)b * cap;
    if (t == 0) { nseg = 0; nvalid = 0; }
    for (int i = t; i < p.sortLen; i += MT_NT) keys[i] = i < n ? ((unsigned long long)(uint32_t)node[i] << 32) | (uint32_t)i : ~0ull;
    if (!side) for (int i = t; i < n; i += MT_NT) a.choice[(size_t)b * cap + i] = -1;
    __syncthreads();
    for (int k = 2; k <= p.sortLen; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < p.sortLen; i += MT_NT) {
                const int o = i ^ j;
                if (o > i) { const unsigned long long x = keys[i], y = keys[o]; if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[o] = x; } }
            }
            __syncthreads();
        }
    for (int i = t; i < n; i += MT_NT) {
        const int nd = (int)(keys[i] >> 32);
        sorted[i] = make_int2(nd, (int)(uint32_t)keys[i]);
        if (nd < 0) continue;                                      // node -1 sorts behind every node
        if (i == n - 1 || (int)(keys[i + 1] >> 32) < 0) nvalid = i + 1;
        if (!side && (i == 0 || (int)(keys[i - 1] >> 32) != nd)) a.segStart[(size_t)b * cap + atomicAdd(&nseg, 1)] = i;      // any order: nodes are independent
    }
    __syncthreads();
    if (t == 0) { a.nValid[side * B + b] = nvalid; if (!side) a.nSeg[b] = nseg; }
}

__device__ __forceinline__ int d_wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int d_lane(int v, int j) { return __builtin_amdgcn_readlane(v, j); }                   // lane j's value, j wave-uniform
__device__ __forceinline__ uint4 d_lane(const uint4 v, int j) { return make_uint4(d_lane((int)v.x, j), d_lane((int)v.y, j), d_lane((int)v.z, j), d_lane((int)v.w, j)); }
__device__ __forceinline__ float d_lane(float v, int j) { return __int_as_float(d_lane(__float_as_int(v), j)); }

// Side A's entries [k0, k1) and side B's nF entries from f0 on, of the node whose first entry in sA is k0.  The three bounds are lower bounds
// (first position whose node is >= key) found by the whole wave in two rounds of loads instead of a bisection's twelve dependent ones: every lane
// probes the first element of one of 64 blocks, then one element of the block the bound falls into; counts are at most BOW_MAX_KEYS = 64 * 64.
struct Seg { int k0, k1, f0, nF; };
__device__ __forceinline__ Seg d_segment(const int2* sA, int nvA, const int2* sB, int nvB, int k0, int lane) {
    const int node = sA[k0].x;
    const int2* s[3] = {sA, sB, sB}; const int n[3] = {nvA, nvB, nvB}, key[3] = {node + 1, node, node + 1};
    int stride[3], v[3], below[3], base[3], r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { stride[i] = (n[i] + 63) >> 6; const int q = lane * stride[i]; v[i] = q < n[i] ? s[i][q].x : 0x7fffffff; }
#pragma unroll
    for (int i = 0; i < 3; i++) { below[i] = __popcll(__ballot(v[i] < key[i])); base[i] = (below[i] - 1) * stride[i]; }      // below > 0: s[base] < key <= s[base + stride]; else the bound is 0
#pragma unroll
    for (int i = 0; i < 3; i++) { const int q = base[i] + 1 + lane; v[i] = (below[i] > 0 && lane < stride[i] && q < n[i]) ? s[i][q].x : 0x7fffffff; }
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = below[i] > 0 ? base[i] + 1 + __popcll(__ballot(v[i] < key[i])) : 0;
    Seg g; g.k0 = k0; g.k1 = r[0]; g.f0 = r[1]; g.nF = r[2] - r[1];
    return g;
}

template <bool KF>
__global__ __launch_bounds__(BW_NT) void k_bow_match(BowParams p, BowArrays a, int B) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (BW_NT / 64) + (threadIdx.x >> 6)), nWaves = gridDim.x * (BW_NT / 64);
    const size_t oa = (size_t)b * p.capA, ob = (size_t)b * p.capB;
    const int2* sA = a.sortedA + oa; const int2* sB = a.sortedB + ob; const int nvA = a.nValid[b], nvB = a.nValid[B + b], nseg = a.nSeg[b];
    const uint8_t* valid = a.flagsA + oa; const uint32_t* dA = a.descA + oa * 8; const uint32_t* dB = a.descB + ob * 8; int* choice = a.choice + oa;
    for (int s = wave; s < nseg; s += nWaves) {
        const Seg g = d_segment(sA, nvA, sB, nvB, a.segStart[oa + s], lane);
        if (g.nF == 0) continue;
        int i0 = 0; uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0;       // the lane's frame keypoint of chunk 0
        if (lane < g.nF) { i0 = sB[g.f0 + lane].y; c0 = *(const uint4*)(dB + 8 * (size_t)i0); c1 = *(const uint4*)(dB + 8 * (size_t)i0 + 4); }
        unsigned long long claimed = 0;                            // bit c: this lane's keypoint of chunk c holds a map point
        if (KF) for (int c = 0, pos = lane; pos < g.nF; c++, pos += 64) if (!a.flagsB[ob + sB[g.f0 + pos].y]) claimed |= 1ull << c;      // pKF2's keypoints without a good map point
        for (int e0 = g.k0; e0 < g.k1; e0 += 64) {                    // 64 entries are loaded by the lanes at once and then taken one after another
            int ikv = 0, okv = 0; uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
            if (e0 + lane < g.k1) { ikv = sA[e0 + lane].y; okv = valid[ikv]; qa = *(const uint4*)(dA + 8 * (size_t)ikv); qb = *(const uint4*)(dA + 8 * (size_t)ikv + 4); }
            const int cnt = min(64, g.k1 - e0);
            for (int j = 0; j < cnt; j++) {
                if (!d_lane(okv, j)) continue;
                const int ik = d_lane(ikv, j); const uint4 q0 = d_lane(qa, j), q1 = d_lane(qb, j);
                int bestD = 256, bestPos = 0, bestIdx = 0, secondD = 256;
                for (int c = 0, pos = lane; c * 64 < g.nF; c++, pos += 64) {
                    if (pos >= g.nF || ((claimed >> c) & 1)) continue;
                    const int idx = c == 0 ? i0 : sB[g.f0 + pos].y;
                    const int dist = c == 0 ? d_hamming(c0, c1, q0, q1) : d_hamming(dB + 8 * (size_t)idx, q0, q1);
                    if (dist < bestD) { secondD = bestD; bestD = dist; bestPos = pos; bestIdx = idx; } else if (dist < secondD) secondD = dist;
                }
                const int key = d_wave_min((bestD << 12) | bestPos), best1 = key >> 12, pos1 = key & (BOW_MAX_KEYS - 1);
                if (KF ? best1 >= TH_LOW : best1 > TH_LOW) continue;
                const bool mine = bestD == best1 && bestPos == pos1;
                const int best2 = d_wave_min(mine ? secondD : bestD);
                if (mine && (float)best1 < p.nnratio * (float)best2) { claimed |= 1ull << (pos1 >> 6); choice[ik] = bestIdx; }
            }
        }
    }
}

__global__ __launch_bounds__(MT_NT) void k_bow_tail(BowParams p, BowArrays a) {
    __shared__ MatchTailShared tail;
    const int b = blockIdx.x, t = threadIdx.x;
    const size_t oa = (size_t)b * p.capA, ob = (size_t)b * p.capB;
    d_assign_and_check_orientation(tail, t, min(a.nA[b], p.capA), min(a.nB[b], p.capB), a.choice + oa, a.matchOfCur + ob, a.angA + oa, a.angB + ob, p.checkOrientation);
    if (t == 0) a.nmatches[b] = tail.nmatch;
}

// what the tests on an idx2 read, per lane
struct TriCand { uint4 d0, d1; float x, y, epi; double sig; int idx, ok, stereo; };

__global__ __launch_bounds__(BW_NT) void k_tri_match(BowParams p, BowArrays a, int B) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (BW_NT / 64) + (threadIdx.x >> 6)), nWaves = gridDim.x * (BW_NT / 64);
    const size_t oa = (size_t)b * p.capA, ob = (size_t)b * p.capB;
    const int2* sA = a.sortedA + oa; const int2* sB = a.sortedB + ob; const int nvA = a.nValid[b], nvB = a.nValid[B + b], nseg = a.nSeg[b];
    const uint8_t* hasMp1 = a.flagsA + oa; const float* xy1 = a.xyA + oa * 2; const float* ur1 = a.urA + oa; const uint32_t* dA = a.descA + oa * 8; int* match12 = a.choice + oa;
    const TriPose& ps = a.pose[b];
    float C2[3];
    d_to_camera(ps.Tcw2, ps.Cw1, C2);
    const float invz = 1.0f / C2[2], ex = p.fx * C2[0] * invz + p.cx, ey = p.fy * C2[1] * invz + p.cy;
    const float* F = ps.F12;
    auto load = [&](int pos) {
        TriCand c; c.idx = sB[pos].y;
        const size_t o = ob + c.idx; const float sc = p.scale[a.octB[o]];
        c.d0 = *(const uint4*)(a.descB + 8 * o); c.d1 = *(const uint4*)(a.descB + 8 * o + 4);
        c.x = a.xyB[2 * o]; c.y = a.xyB[2 * o + 1]; c.epi = 100.f * sc; c.sig = 3.84 * (double)(sc * sc);
        c.stereo = a.urB[o] >= 0; c.ok = !a.flagsB[o] && (c.stereo || !p.onlyStereo);
        return c;
    };
    for (int s = wave; s < nseg; s += nWaves) {
        const Seg g = d_segment(sA, nvA, sB, nvB, a.segStart[oa + s], lane);
        if (g.nF == 0) continue;
        TriCand c0; c0.ok = 0;
        if (lane < g.nF) c0 = load(g.f0 + lane);
        for (int e0 = g.k0; e0 < g.k1; e0 += 64) {                    // 64 entries are loaded by the lanes at once; they are independent of one another
            int i1v = 0, act = 0; float x1v = 0.f, y1v = 0.f; uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
            if (e0 + lane < g.k1) {
                i1v = sA[e0 + lane].y;
                const int stereo1 = ur1[i1v] >= 0;
                act = (!hasMp1[i1v] && (stereo1 || !p.onlyStereo)) ? 1 + stereo1 : 0;       // 0: skipped, 1: mono, 2: stereo
                x1v = xy1[2 * i1v]; y1v = xy1[2 * i1v + 1]; qa = *(const uint4*)(dA + 8 * (size_t)i1v); qb = *(const uint4*)(dA + 8 * (size_t)i1v + 4);
            }
            const int cnt = min(64, g.k1 - e0);
            for (int j = 0; j < cnt; j++) {
                const int act1 = d_lane(act, j);
                if (!act1) continue;
                const bool stereo1 = act1 == 2; const int i1 = d_lane(i1v, j);
                const float x1 = d_lane(x1v, j), y1 = d_lane(y1v, j); const uint4 q0 = d_lane(qa, j), q1 = d_lane(qb, j);
                const float la = x1 * F[0] + y1 * F[3] + F[6], lb = x1 * F[1] + y1 * F[4] + F[7], lc = x1 * F[2] + y1 * F[5] + F[8], den = la * la + lb * lb;
                int best = 0x7fffffff, bestIdx = 0;
                for (int c = 0, pos = lane; c * 64 < g.nF; c++, pos += 64) {
                    if (pos >= g.nF) continue;
                    const TriCand k = c == 0 ? c0 : load(g.f0 + pos);
                    if (!k.ok) continue;
                    const int dist = d_hamming(k.d0, k.d1, q0, q1);
                    if (dist > TH_LOW) continue;
                    if (!stereo1 && !k.stereo) { const float dx = ex - k.x, dy = ey - k.y; if (dx * dx + dy * dy < k.epi) continue; }
                    const float num = la * k.x + lb * k.y + lc;
                    if (den == 0) continue;
                    const float dsqr = num * num / den;
                    if (!((double)dsqr < k.sig)) continue;
                    const int key = (dist << 12) | (BOW_MAX_KEYS - 1 - pos);
                    if (key < best) { best = key; bestIdx = k.idx; }
                }
                const int win = d_wave_min(best);
                if (win != 0x7fffffff && best == win) match12[i1] = bestIdx;        // keys are distinct: one lane writes
            }
        }
    }
}

// vMatches12 is indexed by idx1: count, rotation histogram (kp1.angle - kp2.angle), removal of the bins outside the three maxima
__global__ __launch_bounds__(MT_NT) void k_tri_tail(BowParams p, BowArrays a) {
    __shared__ MatchTailShared sh;
    const int b = blockIdx.x, t = threadIdx.x, n1 = min(a.nA[b], p.capA);
    int* match12 = a.choice + (size_t)b * p.capA; const float* ang1 = a.angA + (size_t)b * p.capA; const float* ang2 = a.angB + (size_t)b * p.capB;
    if (t < HISTO_LENGTH) sh.hist[t] = 0;
    if (t == 0) sh.nmatch = 0;
    __syncthreads();
    for (int i = t; i < n1; i += MT_NT) {
        const int c = match12[i]; if (c < 0) continue;
        atomicAdd(&sh.nmatch, 1);
        if (p.checkOrientation) atomicAdd(&sh.hist[d_rot_bin(ang1[i], ang2[c])], 1);
    }
    __syncthreads();
    if (p.checkOrientation) {
        if (t == 0) d_three_maxima(sh);
        __syncthreads();
        for (int i = t; i < n1; i += MT_NT) {
            const int c = match12[i]; if (c < 0) continue;
            if (!sh.keep[d_rot_bin(ang1[i], ang2[c])]) { match12[i] = -1; atomicAdd(&sh.nmatch, -1); }
        }
        __syncthreads();
    }
    if (t == 0) a.nmatches[b] = sh.nmatch;
}

static int launch_group(const BowParams& p, const BowArrays& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_bow_group, dim3(B, 2), dim3(MT_NT), (size_t)p.sortLen * sizeof(unsigned long long), s, p, a, B);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_match_by_bow(const BowParams& p, const BowArrays& a, int B, hipStream_t s) {
    SIND_TRY(launch_group(p, a, B, s));
    hipLaunchKernelGGL(k_bow_match<false>, dim3(BW_GROUPS, B), dim3(BW_NT), 0, s, p, a, B);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bow_tail, dim3(B), dim3(MT_NT), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_match_by_bow_kf(const BowParams& p, const BowArrays& a, int B, hipStream_t s) {
    SIND_TRY(launch_group(p, a, B, s));
    hipLaunchKernelGGL(k_bow_match<true>, dim3(BW_GROUPS, B), dim3(BW_NT), 0, s, p, a, B);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tri_tail, dim3(B), dim3(MT_NT), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_match_for_triangulation(const BowParams& p, const BowArrays& a, int B, hipStream_t s) {
    SIND_TRY(launch_group(p, a, B, s));
    hipLaunchKernelGGL(k_tri_match, dim3(BW_GROUPS, B), dim3(BW_NT), 0, s, p, a, B);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tri_tail, dim3(B), dim3(MT_NT), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
