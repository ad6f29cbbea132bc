// Sim3Solver::CheckInliers (reference src/Sim3Solver.cc:340-364) with Project (:382-403) for every RANSAC hypothesis of every loop candidate in one launch.
// In Sim3Solver::iterate (:140-207) the sample of iteration k depends only on the random stream and on N (vAvailableIndices = mvAllIndices every time), never
// on an earlier iteration's result, so all mRansacMaxIts (<= 300) hypotheses of all candidates exist before the first inlier test; the reference's "5 iterations
// per candidate, round robin" becomes a replay over the table of counts this kernel writes (sindslam_amd/sim3.py).
//
// What runs where.  The hypothesis itself (ComputeSim3, :226-337: Horn's closed form, a 4x4 Jacobi eigen-solve, cv::Rodrigues) is computed ON THE HOST
// (host/sim3.cpp) and arrives here as T12 / T21.  That is deliberate and not an unfinished port: it calls FP64 atan2, sin and cos, whose device versions do
// not round as glibc's do, bit equality with the restatement is this library's contract, and it is 300 tiny solves per candidate.  The constructor's
// arithmetic (mvX3Dc1/2, mvP1im1, mvP2im2, mvnMaxError1/2; :54-109) is one pass over the correspondences and is done on the host as well.
//
// Shape: one wave per hypothesis, S3_WAVES hypotheses of one candidate per workgroup, lanes stride over the correspondences.  A hypothesis is wave-uniform
// (scalar loads); a correspondence is three float4, one array each, so that every load is 16 B per lane, contiguous.  The inlier mask is the ballot of 64
// correspondences, written by lane 0 with an ordinary store; the count is the sum of the ballots' popcounts.  No atomics, no LDS: a candidate's correspondences
// (48 B each, a few hundred of them in a loop closure) are read by its 300 waves through L2, and staging up to cap of them in LDS would cost a barrier and
// bound cap for nothing.
//
// Arithmetic, per correspondence i and hypothesis (library flags: no contraction, IEEE divide):
//   P3Dc = Rcw * X + tcw               d_to_camera: the small-matrix path of cv::gemm (match_device.hpp)
//   invz = 1 / P3Dc[2]; x = P3Dc[0] * invz; u = fx * x + cx            FP32, in this order
//   dist1 = mvP1im1[i] - vP2im1[i], dist2 = vP1im2[i] - mvP2im2[i]     FP32
//   err = dist.dot(dist)               cv::Mat::dot: the two products and their sum in FP64, then one rounding to float
//   err1 < mvnMaxError1[i] && err2 < mvnMaxError2[i]                   both strict; the bounds are size_t in the reference, converted to float for the comparison
// A NaN hypothesis, z = 0 (invz infinite) and an infinite projection need no special case: every comparison with the resulting NaN or infinity is false.
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

#define S3_WAVES 4

__device__ __forceinline__ void d_sim3_project(const Sim3Params& p, const float* T, const float4 X, float& u, float& v) {
    const float Xw[3] = {X.x, X.y, X.z}; float Pc[3];
    d_to_camera(T, Xw, Pc);
    const float invz = 1 / Pc[2], x = Pc[0] * invz, y = Pc[1] * invz;
    u = p.fx * x + p.cx; v = p.fy * y + p.cy;
}

__device__ __forceinline__ float d_sim3_err(float dx, float dy) { return (float)((double)dx * (double)dx + (double)dy * (double)dy); }

__global__ __launch_bounds__(64 * S3_WAVES) void k_sim3_check(Sim3Params p, Sim3Arrays a) {
    const int b = blockIdx.y, h = blockIdx.x * S3_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (h >= min(a.nIts[b], p.its)) return;                                                          // the whole wave
    const int n = min(a.n[b], p.cap);
    const size_t hq = (size_t)b * p.its + h;
    const Sim3Pose& q = a.hyp[hq];
    float T12[12], T21[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { T12[k] = q.T12[k]; T21[k] = q.T21[k]; }
    const float4* c1 = a.corr + (size_t)b * 3 * p.cap; const float4* c2 = c1 + p.cap; const float4* im = c2 + p.cap;
    unsigned long long* bits = a.bits + hq * p.words;
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {                                                       // ceil(n / 64) <= p.words rounds, the same for every lane
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            const float4 A = c1[i], Bq = c2[i], I = im[i];                                           // (mvX3Dc1, mvnMaxError1), (mvX3Dc2, mvnMaxError2), (mvP1im1, mvP2im2)
            float u, v;
            d_sim3_project(p, T12, Bq, u, v);                                                        // vP2im1
            const float err1 = d_sim3_err(I.x - u, I.y - v);
            d_sim3_project(p, T21, A, u, v);                                                         // vP1im2
            const float err2 = d_sim3_err(u - I.z, v - I.w);
            in = err1 < A.w && err2 < Bq.w;
        }
        const unsigned long long mask = __ballot(in);
        if (lane == 0) bits[base >> 6] = mask;
        cnt += __popcll(mask);
    }
    if (lane == 0) a.count[hq] = cnt;
}

int launch_sim3_check(const Sim3Params& p, const Sim3Arrays& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_sim3_check, dim3(divup(p.its, S3_WAVES), B), dim3(64 * S3_WAVES), 0, s, p, a);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
