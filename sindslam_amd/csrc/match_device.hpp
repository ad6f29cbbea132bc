// Device functions shared by the matcher's searches (match_kernels.hip, match_local.hip, match_bow.hip, bow_kernels.hip): DescriptorDistance
// (reference src/ORBmatcher.cc:1647-1665), and the tail every search with an orientation check ends on -- assignments ->
// CurrentFrame.mvpMapPoints (the later point wins), rotation histogram, ComputeThreeMaxima (:1601-1642), removal.  And the workgroup executor of the two graph
// optimizers (match_localba.hip, match_essgraph.hip).
#pragma once
#include "common.hpp"

namespace sind {

#define MT_NT 1024
#define HISTO_LENGTH 30

// The executor of local_ba and essential_graph for one workgroup of THREADS lanes (host/local_ba.hpp: Ex; the host twins' is SeqExec, host/g2o_lm.hpp): the lanes stride
// over the elements of a phase, then one barrier; a scalar of the control flow is read by every lane, then a barrier, so the next phase may rewrite it
template <int THREADS> struct WgExec {
    int tid;
    template <class F> __device__ void par(int n, F f) {
        for (int i = tid; i < n; i += THREADS) f(i);
        __syncthreads();
    }
    __device__ double rd(const double* p) { const double v = *p; __syncthreads(); return v; }
    __device__ int rdi(const int* p) { const int v = *p; __syncthreads(); return v; }
};

struct MatchTailShared { int hist[HISTO_LENGTH], keep[HISTO_LENGTH], nmatch; };

// bin of the rotation histogram for a match between keypoints of angles a1 and a2 (round(): the product is never negative)
__device__ __forceinline__ int d_rot_bin(float a1, float a2) {
    float rot = a1 - a2; if (rot < 0.0f) rot += 360.0f;
    const int bin = (int)roundf(rot * (1.0f / HISTO_LENGTH));
    return bin == HISTO_LENGTH ? 0 : bin;
}

// ComputeThreeMaxima over sh.hist -> sh.keep (one thread)
__device__ __forceinline__ void d_three_maxima(MatchTailShared& sh) {
    int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = sh.hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; } else if (max3 < 0.1f * (float)max1) ind3 = -1;
    for (int i = 0; i < HISTO_LENGTH; i++) sh.keep[i] = (i == ind1 || i == ind2 || i == ind3);
}

// x3Dc = Rcw * x3Dw + tcw, Tcw = rows 0..2 of the 4x4 pose.  cv::gemm small-matrix path: FP32 row product, FP64 alpha/beta.
__device__ __forceinline__ void d_to_camera(const float* Tcw, const float* X, float* xc) {
    for (int k = 0; k < 3; k++) {
        const float t = Tcw[4 * k] * X[0] + Tcw[4 * k + 1] * X[1] + Tcw[4 * k + 2] * X[2];
        xc[k] = (float)((double)t * 1.0 + (double)Tcw[4 * k + 3] * 1.0);
    }
}

__device__ __forceinline__ int d_hamming(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
__device__ __forceinline__ int d_hamming(const uint32_t* a, const uint4 b0, const uint4 b1) { return d_hamming(*(const uint4*)a, *(const uint4*)(a + 4), b0, b1); }

// choice[i] = current keypoint chosen by point i (-1: none), final.  Called by all MT_NT threads of the workgroup; returns with
// matchOfCur[0..nC) written and sh.nmatch = the function's return value (valid for every thread after the call).
__device__ __forceinline__ void d_assign_and_check_orientation(MatchTailShared& sh, int t, int nL, int nC, const int* choice, int* matchOfCur, const float* lang, const float* cang,
                                                               int checkOrientation) {
    for (int c = t; c < nC; c += MT_NT) matchOfCur[c] = -1;
    if (t < HISTO_LENGTH) sh.hist[t] = 0;
    if (t == 0) sh.nmatch = 0;
    __syncthreads();
    for (int i = t; i < nL; i += MT_NT) {
        const int c = choice[i]; if (c < 0) continue;
        atomicMax(&matchOfCur[c], i); atomicAdd(&sh.nmatch, 1);
        if (checkOrientation) atomicAdd(&sh.hist[d_rot_bin(lang[i], cang[c])], 1);
    }
    __syncthreads();
    if (checkOrientation) {
        if (t == 0) d_three_maxima(sh);
        __syncthreads();
        for (int i = t; i < nL; i += MT_NT) {
            const int c = choice[i]; if (c < 0) continue;
            if (!sh.keep[d_rot_bin(lang[i], cang[c])]) { matchOfCur[c] = -2; atomicAdd(&sh.nmatch, -1); }           // -2 < every index: a removal always wins
        }
        __syncthreads();
        for (int c = t; c < nC; c += MT_NT) if (matchOfCur[c] == -2) matchOfCur[c] = -1;
    }
    __syncthreads();
}

}  // namespace sind
