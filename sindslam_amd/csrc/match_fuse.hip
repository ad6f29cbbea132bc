// The "project map points into a key frame" searches of the local mapper and the loop closer, on the GPU:
//   ORBmatcher::Fuse(pKF, vpMapPoints, th)                          reference src/ORBmatcher.cc:825-975    KF_FUSE
//   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)        :977-1100                              KF_FUSE_SIM3
//   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) :290-403                             KF_PROJ_SIM3
//   ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) :1102-1326                        KF_BY_SIM3
// with KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:569-608), KeyFrame::IsInImage (:610-613) and MapPoint::PredictScale(dist, KeyFrame*)
// (src/MapPoint.cc:385-400).  In three of the four no point depends on another: k_search_kf is a grid over (blocks of KF_NT points) x items,
// one thread per point, projection and window search in one kernel, no rounds, no workgroup per frame; the number of matches is an integer
// atomicAdd.  SearchBySim3 is one launch over 2B items (item 2b + s: the slots of side s of pair b against the keypoints of the other side)
// and k_sim3_agree.  SearchByProjection(pKF, Scw) has the sequential dependence (a keypoint matched by point j is closed for every i > j):
// k_project_kf writes what k_project_points would, and k_search_points<2> (match_local.hip) resolves it in rounds.
// The keypoint record (16 B: x, y, uRight, octave | taken << 16) is packed on the host; as in k_search_points the descriptor is loaded only for
// a candidate that passes every other test and the loads of SR_UNROLL candidates are issued together (profiles/match_local.txt, match_fuse.txt).
// The window is walked in the reference's order (cells x-major, push_back order inside a cell); strict < keeps the first of equal distances.
//
// Arithmetic: items (1)-(7) at the top of match_local.hip.  What differs from Frame::isInFrustum, read off the reference:
//   u = fx * (PcX * invz) + cx        the product with invz comes first here
//   IsInImage                         u >= minX && u < maxX && v >= minY && v < maxY: the upper bounds are strict
//   mnMinX .. mnMaxY                  KeyFrame keeps them as int (include/KeyFrame.h:185-188): the frame's bounds truncated toward zero, on the host; they
//                                     enter IsInImage and GetFeaturesInArea, while mfGridElementWidthInv / HeightInv stay those of the frame's float bounds
//   depth                             PcZ < 0.0f (both Fuse), PcZ < 0.0 in FP64 (the other two)
//   invz                              1 / PcZ in FP32 (KF_FUSE, KF_PROJ_SIM3), (float)(1.0 / PcZ) in FP64 (KF_FUSE_SIM3, KF_BY_SIM3)
//   viewing angle                     PO.dot(Pn) < 0.5 * dist3D compared in FP64 without a division, the dot product accumulated in FP64
//   KF_BY_SIM3                        Pc = sR21 * (R1w * P + t1w) + t21, twice the product of (1); dist3D = cv::norm(Pc) as (3); no viewing angle
//   KF_FUSE, per candidate            ur = u - bf * invz; e2 = ex*ex + ey*ey (+ er*er) in FP32; e2 * mvInvLevelSigma2[kpLevel] in FP32 against the double
//                                     literals 7.8 (mvuRight[idx] >= 0) and 5.99; mvInvLevelSigma2[l] = 1.0f / (scale[l] * scale[l]) (on the host)
//   GetFeaturesInArea                 the key frame's: no level argument, no uRight window test
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

#define KF_NT 64
#define SR_UNROLL 4

struct KfCamera { float fx, fy, cx, cy, minX, maxX, minY, maxY, logScaleFactor; int nlevels; };

// The part of the four functions before GetFeaturesInArea, for one point.  false: the point leaves by one of the reference's `continue`s.
template <int MODE>
__device__ __forceinline__ bool d_project_kf(const KfCamera& c, const float* T, const float* T2, const float* Ow, const float* P, const float* Pn, float maxD, float minD,
                                             float& u, float& v, float& invz, int& lv) {
    float Pc[3];
    d_to_camera(T, P, Pc);
    if (MODE == KF_BY_SIM3) { float q[3]; d_to_camera(T2, Pc, q); Pc[0] = q[0]; Pc[1] = q[1]; Pc[2] = q[2]; }
    if (MODE == KF_FUSE || MODE == KF_FUSE_SIM3) { if (Pc[2] < 0.0f) return false; }
    else if ((double)Pc[2] < 0.0) return false;
    invz = (MODE == KF_FUSE || MODE == KF_PROJ_SIM3) ? 1.0f / Pc[2] : (float)(1.0 / (double)Pc[2]);
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    u = c.fx * x + c.cx; v = c.fy * y + c.cy;
    if (!(u >= c.minX && u < c.maxX && v >= c.minY && v < c.maxY)) return false;                   // a NaN leaves here, as in the reference
    float PO[3];
    if (MODE == KF_BY_SIM3) { PO[0] = Pc[0]; PO[1] = Pc[1]; PO[2] = Pc[2]; }
    else { PO[0] = P[0] - Ow[0]; PO[1] = P[1] - Ow[1]; PO[2] = P[2] - Ow[2]; }
    double s = 0; for (int k = 0; k < 3; k++) s += (double)PO[k] * (double)PO[k];
    const float dist = (float)sqrt(s);
    if (dist < 0.8f * minD || dist > 1.2f * maxD) return false;
    if (MODE != KF_BY_SIM3) {
        double d = 0; for (int k = 0; k < 3; k++) d += (double)PO[k] * (double)Pn[k];
        if (d < 0.5 * (double)dist) return false;
    }
    const float ratio = maxD / dist;
    const float q = ceilf((float)log((double)ratio) / c.logScaleFactor);
    lv = q < 0.f ? 0 : (q >= (float)c.nlevels ? c.nlevels - 1 : (int)q);                            // a NaN falls to (int)NaN = 0
    return true;
}

// KF_FUSE, KF_FUSE_SIM3, KF_BY_SIM3: blockIdx.y = item, one thread per point
template <int MODE>
__global__ __launch_bounds__(KF_NT) void k_search_kf(KfParams p, KfArrays a) {
    const int q = blockIdx.y, i = blockIdx.x * KF_NT + threadIdx.x, n = min(a.nPts[q], p.capPts);
    if (i >= n) return;
    const size_t o = (size_t)q * p.capPts + i;
    a.bestIdx[o] = -1; a.bestDist[o] = -1;
    if (!a.valid[o]) return;
    const KfPose& ps = a.pose[q];
    const KfCamera cam{p.fx, p.fy, p.cx, p.cy, p.bounds[0], p.bounds[1], p.bounds[2], p.bounds[3], p.logScaleFactor, p.nlevels};
    float x, y, invz; int lv;
    if (!d_project_kf<MODE>(cam, ps.T, ps.T2, ps.Ow, a.x3Dw + 3 * o, MODE == KF_BY_SIM3 ? nullptr : a.normal + 3 * o, a.maxDist[o], a.minDist[o], x, y, invz, lv)) return;
    const int kq = MODE == KF_BY_SIM3 ? (q ^ 1) : q;                                               // SearchBySim3 searches the other side of the pair
    const size_t co = (size_t)kq * p.capKeys;
    const float4* pack = a.keyPack + co; const uint32_t* kdesc = a.keyDesc + co * 8; const int* gs = a.gridStart + (size_t)kq * 3073; const int* gi = a.gridIdx + co;
    const float xr = x - p.bf * invz, r = p.th * p.scale[lv];
    const float wInv = p.gridInv[0], hInv = p.gridInv[1];
    const int x0 = max(0, (int)floorf((x - cam.minX - r) * wInv)), x1 = min(63, (int)ceilf((x - cam.minX + r) * wInv));
    const int y0 = max(0, (int)floorf((y - cam.minY - r) * hInv)), y1 = min(47, (int)ceilf((y - cam.minY + r) * hInv));
    if (!(x0 < 64 && x1 >= 0 && y0 < 48 && y1 >= 0)) return;
    const uint4 d0 = *(const uint4*)(a.ptDesc + 8 * o), d1 = *(const uint4*)(a.ptDesc + 8 * o + 4);
    const int minL = lv - 1, maxL = lv;
    int best = -1, bestDist = 256;
    for (int ix = x0; ix <= x1; ix++) {
        const int jb = gs[ix * 48 + y0], je = gs[ix * 48 + y1 + 1];                                // cells (ix, y0..y1) are contiguous in the CSR
        for (int j = jb; j < je; j += SR_UNROLL) {
            int k[SR_UNROLL]; float4 kp[SR_UNROLL];
#pragma unroll
            for (int w = 0; w < SR_UNROLL; w++) k[w] = gi[min(j + w, je - 1)];
#pragma unroll
            for (int w = 0; w < SR_UNROLL; w++) kp[w] = pack[k[w]];
#pragma unroll
            for (int w = 0; w < SR_UNROLL; w++) {
                const int oc = __float_as_int(kp[w].w) & 0xffff;
                int ok = int(j + w < je) & int(oc >= minL) & int(oc <= maxL) & int(fabsf(kp[w].x - x) < r) & int(fabsf(kp[w].y - y) < r);
                if (MODE == KF_FUSE) {
                    const float ex = x - kp[w].x, ey = y - kp[w].y, er = xr - kp[w].z;
                    const bool stereo = kp[w].z >= 0;
                    const float e2 = stereo ? ex * ex + ey * ey + er * er : ex * ex + ey * ey;
                    ok &= int(!((double)(e2 * p.invSigma2[oc]) > (stereo ? 7.8 : 5.99)));
                }
                if (!ok) continue;
                const int dist = d_hamming(kdesc + 8 * k[w], d0, d1);
                if (dist < bestDist) { bestDist = dist; best = k[w]; }
            }
        }
    }
    if (bestDist > p.thDist) return;
    a.bestIdx[o] = best; a.bestDist[o] = bestDist;
    if (MODE != KF_BY_SIM3) atomicAdd(&a.count[q], 1);
}

// SearchBySim3's agreement pass (:1307-1323): bestIdx of items 2b and 2b + 1 are vnMatch1 and vnMatch2
__global__ __launch_bounds__(256) void k_sim3_agree(KfParams p, KfArrays a) {
    const int b = blockIdx.y, i1 = blockIdx.x * 256 + threadIdx.x, n1 = min(a.nPts[2 * b], p.capPts), n2 = min(a.nPts[2 * b + 1], p.capPts);
    if (i1 >= n1) return;
    const int* m1 = a.bestIdx + (size_t)(2 * b) * p.capPts; const int* m2 = m1 + p.capPts;
    const int idx2 = m1[i1];
    const bool agree = idx2 >= 0 && idx2 < n2 && m2[idx2] == i1;
    a.match12[(size_t)b * p.capPts + i1] = agree ? idx2 : -1;
    if (agree) atomicAdd(&a.count[b], 1);
}

// SearchByProjection(pKF, Scw, ...) up to GetFeaturesInArea, into the arrays k_search_points reads
__global__ __launch_bounds__(256) void k_project_kf(LocalParams p, LocalArrays a) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, n = min(a.nPts[b], p.capPts);
    if (i >= n) return;
    const size_t o = (size_t)b * p.capPts + i;
    a.inView[o] = 0; a.projXYR[3 * o] = 0.f; a.projXYR[3 * o + 1] = 0.f; a.projXYR[3 * o + 2] = 0.f; a.level[o] = 0; a.viewCos[o] = 0.f;
    if (!(a.flags[o] & 1)) return;
    const LocalPose& ps = a.pose[b];
    const KfCamera cam{p.fx, p.fy, p.cx, p.cy, p.bounds[0], p.bounds[1], p.bounds[2], p.bounds[3], p.logScaleFactor, p.nlevels};
    float x, y, invz; int lv;
    if (!d_project_kf<KF_PROJ_SIM3>(cam, ps.Tcw, nullptr, ps.Ow, a.x3Dw + 3 * o, a.normal + 3 * o, a.maxDist[o], a.minDist[o], x, y, invz, lv)) return;
    a.inView[o] = 1; a.projXYR[3 * o] = x; a.projXYR[3 * o + 1] = y; a.level[o] = lv;
}

int launch_search_kf(const KfParams& p, const KfArrays& a, int items, int mode, hipStream_t s) {
    const dim3 g(divup(p.capPts, KF_NT), items);
    if (mode == KF_FUSE) hipLaunchKernelGGL(k_search_kf<KF_FUSE>, g, dim3(KF_NT), 0, s, p, a);
    else if (mode == KF_FUSE_SIM3) hipLaunchKernelGGL(k_search_kf<KF_FUSE_SIM3>, g, dim3(KF_NT), 0, s, p, a);
    else hipLaunchKernelGGL(k_search_kf<KF_BY_SIM3>, g, dim3(KF_NT), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_sim3_agree(const KfParams& p, const KfArrays& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_sim3_agree, dim3(divup(p.capPts, 256), B), dim3(256), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_project_kf(const LocalParams& p, const LocalArrays& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_project_kf, dim3(divup(p.capPts, 256), B), dim3(256), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
