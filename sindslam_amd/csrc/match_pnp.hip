// PnPsolver (reference src/PnPsolver.cc): EPnP (compute_pose, :477-525 and what it calls) and CheckInliers (:308-339) for every RANSAC sample of every
// relocalisation candidate in one launch each, and Refine() (:260-305) for the inlier sets that follow from the counts.  In PnPsolver::iterate (:165-258) the
// sample of iteration k depends only on the random stream and on N (vAvailableIndices = mvAllIndices every time), so all samples of all candidates exist before
// the first inlier test; the reference's "5 iterations per candidate, round robin" becomes a replay over the table of counts (sindslam_amd/pnp.py).
//
// What runs where.  Unlike Sim3Solver's Horn solve (match_sim3.hip), the hypothesis is computed HERE: an EPnP solve is a 12 x 12 Jacobi SVD, three small SVD
// solves, fifteen QR solves and three 3 x 3 SVDs in FP64, hundreds of times heavier than a Horn solve, and it calls nothing but add, mul, div, sqrt and fabs, which
// the device rounds as the host does.  host/epnp.hpp is the one source of it for both sides (hypot is defined there, not taken from ocml); the library's flags
// forbid contraction.  The device result is compared with the host's bit for bit (tests/test_pnp_gpu.py).
//
// Shapes.  k_pnp_pose4: one sample per lane, everything in private memory: the 12 x 12 matrix the SVD rotates in place (1152 B) and the small systems are indexed
// dynamically, so they live in scratch, which the hardware interleaves across the lanes of a wave as an [element][lane] layout in LDS would; see
// profiles/match_pnp_ransac.txt for what the compiler reports.  k_pnp_pose_set: one Refine problem per lane; its n-sized arrays (pws, us, alphas, pcs) are in a
// global workspace of the handle, [element][slot], so the lanes of a wave read neighbouring words.  k_pnp_check: one wave per pose, lanes stride over
// the correspondences, the inlier mask is the ballot of 64 of them written by lane 0, the count the sum of popcounts.  No atomics, no LDS.
// CheckInliers' mixed precision is epnp_is_inlier's: Xc, Yc FP64 expressions rounded to float, invZc the float of an FP64 quotient, ue, ve FP64, distX, distY, error2 float,
// strict < against the float bound.  A NaN pose and Zc == 0 need no special case: every comparison with the resulting NaN or infinity is false.
#include "match.hpp"
#include "host/epnp.hpp"

namespace sind {

#define PNP_WAVES 4

__global__ __launch_bounds__(64) void k_pnp_pose4(PnpParams p, PnpArrays a, int B) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= B * p.its) return;
    const int b = q / p.its, h = q - b * p.its;
    if (h >= min(a.nIts[b], p.its)) return;
    const int4 sm = a.samples[q];
    const int idx[4] = {sm.x, sm.y, sm.z, sm.w};
    const int n = min(a.n[b], p.cap);
    if (n < 1) return;
    double pws[12], us[8], ws[28], mtm[144], R[3][3], t[3];
    for (int k = 0; k < 4; k++) {
        const int i = min(max(idx[k], 0), n - 1);                                                    // the host has checked the range; never outside the candidate's rows
        const float4 P = a.pts[(size_t)b * p.cap + i]; const float2 U = a.uv[(size_t)b * p.cap + i];
        pws[3 * k] = P.x; pws[3 * k + 1] = P.y; pws[3 * k + 2] = P.z; us[2 * k] = U.x; us[2 * k + 1] = U.y;
    }
    epnp_compute_pose(4, pws, us, 1, p.fu, p.fv, p.uc, p.vc, ws, mtm, R, t);
    PnpPose& o = a.pose[q];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) o.R[3 * i + j] = R[i][j]; o.t[i] = t[i]; }
}

__global__ __launch_bounds__(PNP_REFINE_SLOTS) void k_pnp_pose_set(PnpParams p, PnpArrays a, int nRefines) {
    const int slot = threadIdx.x;
    if (slot >= nRefines || slot >= PNP_REFINE_SLOTS) return;
    const PnpRefine r = a.refine[slot];
    const int n = min(a.n[r.b], p.cap);
    const unsigned long long* bits = r.hyp < 0 ? a.bestBits + (size_t)r.b * p.words : a.bits + ((size_t)r.b * p.its + r.hyp) * p.words;
    const int S = PNP_REFINE_SLOTS;
    double* pws = a.work + slot; double* us = pws + (size_t)3 * p.cap * S; double* ws = us + (size_t)2 * p.cap * S;
    int m = 0;
    for (int i = 0; i < n; i++) {                                                                    // Refine's vIndices (:265-281), ascending
        if (!((bits[i >> 6] >> (i & 63)) & 1ull)) continue;
        const float4 P = a.pts[(size_t)r.b * p.cap + i]; const float2 U = a.uv[(size_t)r.b * p.cap + i];
        pws[(size_t)(3 * m) * S] = P.x; pws[(size_t)(3 * m + 1) * S] = P.y; pws[(size_t)(3 * m + 2) * S] = P.z;
        us[(size_t)(2 * m) * S] = U.x; us[(size_t)(2 * m + 1) * S] = U.y;
        m++;
    }
    double mtm[144], R[3][3], t[3];
    epnp_compute_pose(m, pws, us, S, p.fu, p.fv, p.uc, p.vc, ws, mtm, R, t);
    PnpPose& o = a.refPose[slot];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) o.R[3 * i + j] = R[i][j]; o.t[i] = t[i]; }
}

// refines = 0: pose q = sample h of candidate b, q = b * its + h; else pose q = this round's Refine problem q
__global__ __launch_bounds__(64 * PNP_WAVES) void k_pnp_check(PnpParams p, PnpArrays a, int nPoses, int refines) {
    const int q = blockIdx.x * PNP_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (q >= nPoses) return;                                                                         // the whole wave
    int b;
    if (refines) b = a.refine[q].b;
    else { b = q / p.its; if (q - b * p.its >= min(a.nIts[b], p.its)) return; }
    const int n = min(a.n[b], p.cap);
    const PnpPose& P = refines ? a.refPose[q] : a.pose[q];
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = P.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = P.t[k];
    const float4* pts = a.pts + (size_t)b * p.cap; const float2* uv = a.uv + (size_t)b * p.cap;
    unsigned long long* bits = (refines ? a.refBits : a.bits) + (size_t)q * p.words;
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {                                                       // ceil(n / 64) <= p.words rounds, the same for every lane
        const int i = base + lane;
        bool in = false;
        if (i < n) { const float4 X = pts[i]; const float2 U = uv[i]; in = epnp_is_inlier(R, t, p.fu, p.fv, p.uc, p.vc, X.x, X.y, X.z, U.x, U.y, X.w); }
        const unsigned long long mask = __ballot(in);
        if (lane == 0) bits[base >> 6] = mask;
        cnt += __popcll(mask);
    }
    if (lane == 0) (refines ? a.refCount : a.count)[q] = cnt;
}

int launch_pnp_samples(const PnpParams& p, const PnpArrays& a, int B, hipStream_t s) {
    const int nq = B * p.its;
    hipLaunchKernelGGL(k_pnp_pose4, dim3(divup(nq, 64)), dim3(64), 0, s, p, a, B);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_check, dim3(divup(nq, PNP_WAVES)), dim3(64 * PNP_WAVES), 0, s, p, a, nq, 0);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_pnp_refines(const PnpParams& p, const PnpArrays& a, int nRefines, hipStream_t s) {
    hipLaunchKernelGGL(k_pnp_pose_set, dim3(1), dim3(PNP_REFINE_SLOTS), 0, s, p, a, nRefines);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_check, dim3(divup(nRefines, PNP_WAVES)), dim3(64 * PNP_WAVES), 0, s, p, a, nRefines, 1);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
