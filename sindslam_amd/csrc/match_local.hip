// The two projection searches of the RGB-D tracker whose points are map points, on the GPU:
//   Tracking::SearchLocalPoints: Frame::isInFrustum (reference src/Frame.cc:340-396) + MapPoint::PredictScale (src/MapPoint.cc:402-418)
//     for every local map point, then ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:45-137);
//   Tracking::Relocalization: ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1472-1599).
// k_project_points: one thread per point, B frames per launch; its outputs stay on the device for k_search_points: one workgroup
// per frame, one thread per point, the round scheme of match_kernels.hip for the one sequential dependence (a keypoint is closed
// for point i exactly when some j < i that closes keypoints chose it; closed candidates are skipped before the distance, so they
// never enter best / second best).  The window is walked in the reference's order (cells x-major, push_back order inside a cell).
// The camera transform, the Hamming distance and the orientation tail are match_device.hpp's, shared with match_kernels.hip.
// Shape and loop form were measured once, profiles/match_local.txt; nothing was tuned beyond that.
//
// Arithmetic (FP32 unless said; -ffp-contract=off, IEEE division):
//   Pc = Rcw * P + tcw       FP32 row product, then (float)((double)t + (double)tcw[r])                    parity UNPINNED (1)
//   invz                     isInFrustum: 1.0f / PcZ in FP32 after rejecting PcZ < 0; relocalisation: (float)(1.0 / PcZ) in FP64, no sign test
//   Ow = -Rcw^T * tcw        FP64 accumulation, times -1, to FP32 (on the host, once per frame)             parity UNPINNED (2)
//   dist = |P - Ow|          FP32 difference, squares summed in FP64, (float)sqrt                          parity UNPINNED (3)
//   viewCos                  (float)(sum (double)PO_k * (double)Pn_k / (double)dist)                        parity UNPINNED (4)
//   PredictScale             ratio = mfMaxDistance / dist; ceil(log(ratio) / mfLogScaleFactor) clamped to 0 .. nlevels-1, where
//                            log is DEFINED as the FP64 logarithm rounded to FP32 (a correctly rounded logf but for midpoint cases
//                            of probability ~2^-29), here for ratio and on the host for mfLogScaleFactor = log(mvScaleFactors[1]).
//                            The reference calls the FP32 std::log, whose last bit differs between C libraries, and that bit
//                            decides the level of a point seen again at the distance it was created at (ratio == scale[octave]).
//   A / s, s * A             (Scw decomposition, sR12, sR21 of match_fuse.hip, on the host) every element times (float)(1.0 / (double)s), resp. (float)s,
//                            in FP32: a MatExpr with a scale factor, evaluated by convertTo                  parity UNPINNED (5)
//   scw                      (float)sqrt(row0 . row0), the dot product as in (4): FP64 accumulation          parity UNPINNED (6)
//   t21 = -sR21 * t12        FP32 row product, then (float)((double)t * -1.0): the alpha of (1)              parity UNPINNED (7)
//   Ow of an Scw             -Rcw^T * tcw as (2), on Rcw and tcw of (5)
// (1)-(7) are recollections of OpenCV 4.2.0 (cv::gemm small-matrix path, cv::gemm with GEMM_1_T, cv::norm of a CV_32F matrix,
// Mat::dot returning double, MatExpr scaling through convertTo) that nothing in this repository can pin.
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

#define PP_NT 256
#define SR_UNROLL 4

template <bool RELOC>
__global__ __launch_bounds__(PP_NT) void k_project_points(LocalParams p, LocalArrays a) {
    const int b = blockIdx.y, i = blockIdx.x * PP_NT + threadIdx.x, n = min(a.nPts[b], p.capPts);
    if (i >= n) return;
    const size_t o = (size_t)b * p.capPts + i;
    a.inView[o] = 0; a.projXYR[3 * o] = 0.f; a.projXYR[3 * o + 1] = 0.f; a.projXYR[3 * o + 2] = 0.f; a.level[o] = 0; a.viewCos[o] = 0.f;
    if (!(a.flags[o] & 1)) return;
    const LocalPose& ps = a.pose[b];
    const float* P = a.x3Dw + 3 * o;
    float Pc[3];
    d_to_camera(ps.Tcw, P, Pc);
    float invz;
    if (RELOC) invz = (float)(1.0 / Pc[2]);
    else { if (Pc[2] < 0.0f) return; invz = 1.0f / Pc[2]; }
    const float u = p.fx * Pc[0] * invz + p.cx, v = p.fy * Pc[1] * invz + p.cy;
    if (u < p.bounds[0] || u > p.bounds[1]) return;
    if (v < p.bounds[2] || v > p.bounds[3]) return;
    const float PO[3] = {P[0] - ps.Ow[0], P[1] - ps.Ow[1], P[2] - ps.Ow[2]};
    double s = 0; for (int k = 0; k < 3; k++) s += (double)PO[k] * (double)PO[k];
    const float dist = (float)sqrt(s);
    const float maxD = a.maxDist[o];
    if (dist < 0.8f * a.minDist[o] || dist > 1.2f * maxD) return;
    float viewCos = 0.f;
    if (!RELOC) {
        const float* Pn = a.normal + 3 * o;
        double d = 0; for (int k = 0; k < 3; k++) d += (double)PO[k] * (double)Pn[k];
        viewCos = (float)(d / (double)dist);
        if (viewCos < p.viewCosLimit) return;
    }
    const float ratio = maxD / dist;
    const float q = ceilf((float)log((double)ratio) / p.logScaleFactor);
    const int lv = q < 0.f ? 0 : (q >= (float)p.nlevels ? p.nlevels - 1 : (int)q);             // a NaN falls to (int)NaN = 0
    a.inView[o] = 1; a.projXYR[3 * o] = u; a.projXYR[3 * o + 1] = v; a.projXYR[3 * o + 2] = u - p.bf * invz; a.level[o] = lv; a.viewCos[o] = viewCos;
    if (!RELOC) atomicAdd(&a.nToMatch[b], 1);
}

// MODE 0: local map, 1: relocalisation, 2: SearchByProjection(pKF, Scw, ...) after k_project_kf (match_fuse.hip): the relocalisation search with levels [lv-1, lv],
// TH_LOW in orbDist, the key frame's int bounds in p.bounds and its grid cell size in p.gridInv
template <int MODE>
__global__ __launch_bounds__(MT_NT) void k_search_points(LocalParams p, LocalArrays a) {
    constexpr bool RELOC = MODE != 0;
    __shared__ int changed; __shared__ MatchTailShared tail;
    const int b = blockIdx.x, t = threadIdx.x, nP = min(a.nPts[b], p.capPts), nC = min(a.nCur[b], p.capCur);
    const size_t po = (size_t)b * p.capPts, co = (size_t)b * p.capCur;
    const uint8_t* flags = a.flags + po; const uint8_t* inView = a.inView + po; const float* proj = a.projXYR + po * 3; const int* level = a.level + po;
    const float* viewCos = a.viewCos + po; const uint32_t* pdesc = a.ptDesc + po * 8;
    const float* cxy = a.curUnXY + co * 2; const int* coct = a.curOctave + co; const float* cur = a.curURight + co; const uint32_t* cdesc = a.curDesc + co * 8;
    const int* gs = a.gridStart + (size_t)b * 3073; const int* gi = a.gridIdx + co; const uint8_t* taken0 = a.curTaken + co;
    int* choice = a.choice + po; int* minOwner = a.minOwner + co; int* matchOfCur = a.matchOfCur + co; float4* pack = a.curPack + co;
    const float minX = p.bounds[0], minY = p.bounds[2];
    const float wInv = MODE == 2 ? p.gridInv[0] : 64.f / (float)(p.bounds[1] - p.bounds[0]), hInv = MODE == 2 ? p.gridInv[1] : 48.f / (float)(p.bounds[3] - p.bounds[2]);
    const int thHigh = RELOC ? p.orbDist : 100;

    for (int i = t; i < nP; i += MT_NT) choice[i] = -1;
    for (int c = t; c < nC; c += MT_NT)                                                           // keypoint record: x, y, uRight, octave | taken << 16
        pack[c] = make_float4(cxy[2 * c], cxy[2 * c + 1], RELOC ? 0.f : cur[c], __int_as_float((coct[c] & 0xffff) | (taken0[c] ? 0x10000 : 0)));
    int round = 0;
    for (;;) {
        for (int c = t; c < nC; c += MT_NT) minOwner[c] = 0x7fffffff;
        if (t == 0) changed = 0;
        __syncthreads();
        for (int i = t; i < nP; i += MT_NT) { const int c = choice[i]; if (c >= 0 && (flags[i] & 2)) atomicMin(&minOwner[c], i); }
        __syncthreads();
        for (int i = t; i < nP; i += MT_NT) {
            int best = -1;
            if (inView[i]) {
                const int lv = level[i];
                float r;
                if (RELOC) r = p.th * p.scale[lv];
                else {
                    r = (double)viewCos[i] > 0.998 ? 2.5f : 4.0f;                                  // RadiusByViewingCos compares against a double literal
                    if (p.th != 1.0f) r *= p.th;
                    r = r * p.scale[lv];
                }
                const int minL = lv - 1, maxL = MODE == 1 ? lv + 1 : lv;                              // maxL >= 0: levels are always checked
                const float x = proj[3 * i], y = proj[3 * i + 1], xr = proj[3 * i + 2];
                const int x0 = max(0, (int)floorf((x - minX - r) * wInv)), x1 = min(63, (int)ceilf((x - minX + r) * wInv));
                const int y0 = max(0, (int)floorf((y - minY - r) * hInv)), y1 = min(47, (int)ceilf((y - minY + r) * hInv));
                if (x0 < 64 && x1 >= 0 && y0 < 48 && y1 >= 0) {
                    const uint4 d0 = *(const uint4*)(pdesc + 8 * i), d1 = *(const uint4*)(pdesc + 8 * i + 4);
                    int bestDist = 256, bestDist2 = 256, bestLevel = -1, bestLevel2 = -1;
                    for (int ix = x0; ix <= x1; ix++) {
                        const int jb = gs[ix * 48 + y0], je = gs[ix * 48 + y1 + 1];               // cells (ix, y0..y1) are contiguous in the CSR
                        // The loop is bound by the latency of its dependent loads (grid index -> keypoint -> descriptor) at 16 waves on one CU.
                        // So: one 16 B record per keypoint instead of five scalars, the loads of SR_UNROLL candidates issued together and the
                        // candidates then tested in order, the descriptor only for one that passes every test (profiles/match_local.txt).
                        for (int j = jb; j < je; j += SR_UNROLL) {
                            int k[SR_UNROLL], owner[SR_UNROLL]; float4 kp[SR_UNROLL];
#pragma unroll
                            for (int u = 0; u < SR_UNROLL; u++) k[u] = gi[min(j + u, je - 1)];
#pragma unroll
                            for (int u = 0; u < SR_UNROLL; u++) { kp[u] = pack[k[u]]; owner[u] = minOwner[k[u]]; }
#pragma unroll
                            for (int u = 0; u < SR_UNROLL; u++) {
                                const int meta = __float_as_int(kp[u].w), oc = meta & 0xffff;
                                int ok = int(j + u < je) & int(oc >= minL) & int(oc <= maxL) & int(fabsf(kp[u].x - x) < r) & int(fabsf(kp[u].y - y) < r) & int(!(meta >> 16)) &
                                         int(!(owner[u] < i));
                                if (!RELOC) ok &= int(!(kp[u].z > 0 && fabsf(xr - kp[u].z) > r));
                                if (!ok) continue;
                                const int dist = d_hamming(cdesc + 8 * k[u], d0, d1);
                                if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = oc; best = k[u]; }
                                else if (dist < bestDist2) { bestLevel2 = oc; bestDist2 = dist; }
                            }
                        }
                    }
                    if (bestDist > thHigh) best = -1;
                    else if (!RELOC && bestLevel == bestLevel2 && (float)bestDist > p.nnratio * (float)bestDist2) best = -1;
                }
            }
            if (best != choice[i]) { choice[i] = best; changed = 1; }
        }
        __syncthreads();
        round++;
        const int ch = changed;
        __syncthreads();
        if (!ch || round > nP) break;
    }
    d_assign_and_check_orientation(tail, t, nP, nC, choice, matchOfCur, a.ptAngle + po, a.curAngle + co, RELOC ? p.checkOrientation : 0);
    if (t == 0) { a.nmatches[b] = tail.nmatch; a.rounds[b] = round; }
}

int launch_project_points(const LocalParams& p, const LocalArrays& a, int B, int reloc, hipStream_t s) {
    const dim3 g(divup(p.capPts, PP_NT), B);
    if (reloc) hipLaunchKernelGGL(k_project_points<true>, g, dim3(PP_NT), 0, s, p, a);
    else hipLaunchKernelGGL(k_project_points<false>, g, dim3(PP_NT), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_search_points(const LocalParams& p, const LocalArrays& a, int B, int mode, hipStream_t s) {
    if (mode == 2) hipLaunchKernelGGL(k_search_points<2>, dim3(B), dim3(MT_NT), 0, s, p, a);
    else if (mode) hipLaunchKernelGGL(k_search_points<1>, dim3(B), dim3(MT_NT), 0, s, p, a);
    else hipLaunchKernelGGL(k_search_points<0>, dim3(B), dim3(MT_NT), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
