// The flow-mask stage: flow magnitude and homography residual, their histogram, the Otsu and Triangle thresholds, the two masks -- per frame and for the
// frames of a record table.
#include "flow_dev.hpp"

namespace sind {

// ---------------------------------------------------------------------------------------------------------
// Large-motion test, reference DynaDetect.cc:1081-1114: magnitude, max, u8 normalisation, 256-bin histogram.
// Pass 1: per-image max of |flow| (non-negative floats order like their bit patterns -> integer atomicMax).
__global__ void k_mag_max(const float* __restrict__ u, const float* __restrict__ v, float* __restrict__ mag, unsigned* __restrict__ maxbits, int n) {
    const int b = blockIdx.y;
    float m = 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float x = u[(size_t)b * n + i], y = v[(size_t)b * n + i];
        const float g = sqrtf(x * x + y * y);
        if (mag) mag[(size_t)b * n + i] = g;
        m = fmaxf(m, g);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(&maxbits[b], __float_as_uint(m));
}
// Pass 2: histogram of saturate_cast<uchar>(mag * (float)(255.0/max)); LDS histogram per workgroup, one global
// atomic per bin per workgroup.  Optionally stores the u8 image (residual stage).
__device__ __forceinline__ void mag_hist_plane(const float* __restrict__ mag, const unsigned* __restrict__ maxbits, int* __restrict__ hist,
                                               uint8_t* __restrict__ out_u8, int n, int* lh) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) lh[i] = 0;
    __syncthreads();
    const float a = (float)(255.0 / (double)__uint_as_float(*maxbits));
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int q = d_cvRound(mag[i] * a);
        q = min(max(q, 0), 255);
        if (out_u8) out_u8[i] = (uint8_t)q;
        atomicAdd(&lh[q], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += blockDim.x) if (lh[i]) atomicAdd(&hist[i], lh[i]);
}
__global__ void k_mag_hist(const float* __restrict__ mag, const unsigned* __restrict__ maxbits, int* __restrict__ hist,
                           uint8_t* __restrict__ out_u8, int n) {
    __shared__ int lh[256];
    const int b = blockIdx.y;
    mag_hist_plane(mag + (size_t)b * n, maxbits + b, hist + b * 256, out_u8 ? out_u8 + (size_t)b * n : nullptr, n, lh);
}
// the same for the frames of a record table (flow-mask stage of a whole k-means group): blockIdx.y = record
__global__ void k_mag_hist_frames(const FlowMaskRec* __restrict__ recs, int n) {
    __shared__ int lh[256];
    const FlowMaskRec& R = recs[blockIdx.y];
    mag_hist_plane(R.mag, reinterpret_cast<const unsigned*>(R.hist + 256), R.hist, R.magu8, n, lh);
}

// ---------------------------------------------------------------------------------------------------------
// Residual stage, reference DynaDetect.cc:1252-1271: flow - (p - H p), homography part in FP64 then cast to FP32.
// A thread takes RM_ROWS pixels of one column (2 400 workgroups of one row segment each were mostly workgroup turnover: 11 us of the whole GPU per 640 x 480 frame, 512 times a step)
#define RM_ROWS 4
__device__ __forceinline__ void residual_mag_rows(const float* __restrict__ u, const float* __restrict__ v, const double* __restrict__ H, float* __restrict__ mag,
                                                  unsigned* __restrict__ maxbits, int w, int h, int col, int row0) {
    float m = 0.f;
    if (col < w) {
        #pragma unroll
        for (int r = 0; r < RM_ROWS; r++) {
            const int row = row0 + r;
            if (row >= h) break;
            const double den = H[6] * col + H[7] * row + H[8];
            const double fx2 = (col - (H[0] * col + H[1] * row + H[2]) / den);
            const double fy2 = (row - (H[3] * col + H[4] * row + H[5]) / den);
            const float dx = u[row * w + col] - (float)fx2, dy = v[row * w + col] - (float)fy2;
            const float mm = sqrtf(dx * dx + dy * dy);
            mag[row * w + col] = mm;
            m = fmaxf(m, mm);
        }
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    // thousands of waves hitting one address serialise in L2: a wave only issues the atomic when it can still raise the maximum
    if ((threadIdx.x & 63) == 0 && __float_as_uint(m) > *(volatile unsigned*)maxbits) atomicMax(maxbits, __float_as_uint(m));
}
__global__ void k_residual_mag(const float* __restrict__ u, const float* __restrict__ v, HMat Hm, float* __restrict__ mag,
                               unsigned* __restrict__ maxbits, int w, int h) {
    residual_mag_rows(u, v, Hm.h, mag, maxbits, w, h, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y * RM_ROWS);
}
// the same for the frames of a record table: blockIdx.z = record, the homography comes from the record
__global__ void k_residual_mag_frames(const FlowMaskRec* __restrict__ recs, int w, int h) {
    const FlowMaskRec& R = recs[blockIdx.z];
    residual_mag_rows(R.U, R.V, R.H, R.mag, reinterpret_cast<unsigned*>(R.hist + 256), w, h, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y * RM_ROWS);
}
// The two thresholds of stImgMasks from the residual's 256-bin histogram, on the device so that the flow-mask stage needs ONE host round trip (masks,
// histogram and thresholds come back together): cv::threshold's THRESH_OTSU / THRESH_TRIANGLE return values (imgproc/thresh.cpp) and the clamping of
// DD:1309-1367, with the host code's FP64 / FP32 operations in the same order (no contraction: the library is built with -ffp-contract=off).
// k_flow_thresholds_serial is the one-thread statement of it (83 us per frame: every iteration of Otsu's loop carries an FP64 division) and stays as the
// in-library reference; k_flow_thresholds gives the same bits from ONE WAVE:
//   * sums of integers below 2^53 (the mean, Triangle's distances, the pixel counts) are exact in FP64 in any order -> lane-parallel + wave reduction;
//   * q1 += p_i is a rounding chain -> walked in order, but it does not depend on mu1, so it runs first (one dependent add per bin);
//   * mu1 = (mu1 * q1_old + i * p_i) / q1 is the only chain with a division: the divisor q1_i is known beforehand, so every lane prepares the refined
//     reciprocal y_i of its four bins with the compiler's own FP64 division sequence (v_rcp_f64 + two Newton steps), and the chain keeps only that
//     sequence's last three operations (q0 = n y, r = fma(-q1, q0, n), q = fma(r, y, q0)); operands are far from the exponent range where
//     v_div_scale / v_div_fixup would act (q1 in [1.2e-7, 1], n in [0, 255]);
//   * sigma, its arg max (first maximum wins, like the sequential `>` test) and Triangle's arg max are lane-parallel again.
// hist: [256] counts + [256] = bit pattern of the maximal residual; res: [261] = the same 257 words + lo, hi, otsu, triangle; the kernel leaves hist
// ZEROED for the next frame (the residual kernels accumulate into it).  dbg_mu1 (optional): the 256 values of the mu1 chain.  One block = one histogram.
__global__ void k_flow_thresholds_serial(const int* __restrict__ hist, int W, int H, float* __restrict__ out) {
    hist += (size_t)blockIdx.x * 257; out += (size_t)blockIdx.x * 4;
    if (threadIdx.x != 0) return;
    const int N = W * H;
    const float maxErrorf = __int_as_float(hist[256]);
    double otsu_v;
    {
        double mu = 0; const double scale = 1. / N;
        for (int i = 0; i < 256; i++) mu += i * (double)hist[i];
        mu *= scale;
        double mu1 = 0, q1 = 0, max_sigma = 0, max_val = 0;
        for (int i = 0; i < 256; i++) {
            const double p_i = hist[i] * scale; mu1 *= q1; q1 += p_i; const double q2 = 1. - q1;
            if (fmin(q1, q2) < (double)1.1920928955078125e-7f || fmax(q1, q2) > 1. - (double)1.1920928955078125e-7f) continue;
            mu1 = (mu1 + i * p_i) / q1; const double mu2 = (mu - q1 * mu1) / q2, sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
            if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
        }
        otsu_v = max_val;
    }
    double tri_v;
    {
        int left = 0, right = 0, max_ind = 0, mx = 0; bool flipped = false;
        for (int i = 0; i < 256; i++) if (hist[i] > 0) { left = i; break; }
        if (left > 0) left--;
        for (int i = 255; i > 0; i--) if (hist[i] > 0) { right = i; break; }
        if (right < 255) right++;
        for (int i = 0; i < 256; i++) if (hist[i] > mx) { mx = hist[i]; max_ind = i; }
        if (max_ind - left < right - max_ind) { flipped = true; left = 255 - right; max_ind = 255 - max_ind; }
        double thresh = left, a = mx, b = left - max_ind, dist = 0;
        for (int i = left + 1; i <= max_ind; i++) { const double t = a * i + b * hist[flipped ? 255 - i : i]; if (t > dist) { dist = t; thresh = i; } }
        thresh--;
        if (flipped) thresh = 255 - thresh;
        tri_v = thresh;
    }
    float thred1 = (float)otsu_v, thred2 = (float)tri_v;
    out[2] = thred1; out[3] = thred2;
    auto count_gt = [&](float t) { int n = 0; for (int v = 0; v < 256; v++) if ((double)v > (double)t) n += hist[v]; return n; };
    float lo, hi;
    if (thred1 < thred2) {                                    // DD:1309-1336
        if (thred1 < 1.7f * 255.0f / maxErrorf) thred1 = 1.7f * 255.0f / maxErrorf;
        else if (thred1 > 3.0f * 255.0f / maxErrorf) thred1 = 3.0f * 255.0f / maxErrorf;
        if (count_gt(thred1) > 0.5 * W * H) thred1 = thred1 + 0.2f * 255.0f / maxErrorf;
        if (thred2 < fmaxf(3.0f * 255.0f / maxErrorf, thred1 * 1.2f)) thred2 = fmaxf(3.0f * 255.0f / maxErrorf, thred1 * 1.2f);
        else if (thred2 > 10.0f * 255.0f / maxErrorf) thred2 = 10.0f * 255.0f / maxErrorf;
        lo = thred1; hi = thred2;
    } else {                                                  // DD:1337-1367 (the relaxation test there is dead code)
        if (thred2 < 1.7f * 255.0f / maxErrorf) thred2 = 1.7f * 255.0f / maxErrorf;
        else if (thred2 > 3.0f * 255.0f / maxErrorf) thred2 = 3.0f * 255.0f / maxErrorf;
        if (thred1 < fmaxf(3.0f * 255.0f / maxErrorf, thred2 * 1.2f)) thred1 = fmaxf(3.0f * 255.0f / maxErrorf, thred2 * 1.2f);
        else if (thred1 > 10.0f * 255.0f / maxErrorf) thred1 = 10.0f * 255.0f / maxErrorf;
        lo = thred2; hi = thred1;
    }
    out[0] = lo; out[1] = hi;
}

__device__ __forceinline__ double wave_sum_f64(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }      // exact when every partial sum is an integer below 2^53
__device__ __forceinline__ int wave_sum_i32(int v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ int wave_min_i32(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ int wave_max_i32(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }
// arg max with "first maximum wins": larger value, on equal values the smaller index
__device__ __forceinline__ void wave_argmax_f64(double& v, int& idx) {
    for (int o = 32; o > 0; o >>= 1) { const double ov = __shfl_xor(v, o); const int oi = __shfl_xor(idx, o); if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; } }
}
__device__ __forceinline__ void flow_thresholds_wave(int* __restrict__ hist, int W, int H, int* __restrict__ res, double* __restrict__ dbg_mu1, int keep_hist,
                                                     double* s_p, double4* s_c) {
    const int lane = threadIdx.x, N = W * H;
    const int4 h4 = *reinterpret_cast<const int4*>(hist + 4 * lane);
    const int hmax_bits = hist[256];
    const int h[4] = {h4.x, h4.y, h4.z, h4.w};
    // result block (the working histogram is zeroed at the very end, when every lane's loads have long been consumed)
    *reinterpret_cast<int4*>(res + 4 * lane) = h4; if (lane == 0) res[256] = hmax_bits;
    const float maxErrorf = __int_as_float(hmax_bits);
    // ---- Otsu
    const double scale = 1. / N;
    double mu = 0, pv[4];
    #pragma unroll
    for (int k = 0; k < 4; k++) { mu += (4 * lane + k) * (double)h[k]; pv[k] = h[k] * scale; s_p[4 * lane + k] = pv[k]; }
    mu = wave_sum_f64(mu) * scale;
    __syncthreads();
    // The chains below are walked by every lane (wave-uniform values); a lane keeps the four values of its own bins.  No LDS store inside the loops: the
    // loads of the coming bins do not depend on the chain and must be free to move ahead of it (an LDS store in between pins them behind it: measured
    // 37 us for the kernel with the stores, the LDS latency then sits on the chain 512 times).
    double q1v[4] = {0, 0, 0, 0};
    {   // q1 chain (same hand pipelining as the mu1 chain below)
        double q1 = 0;
        double4 cur = *reinterpret_cast<const double4*>(&s_p[0]), nxt;
        for (int L = 0; L < 64; L++) {
            nxt = *reinterpret_cast<const double4*>(&s_p[4 * min(L + 1, 63)]);
            __builtin_amdgcn_sched_barrier(0);
            const bool mine = L == lane;
            q1 += cur.x; if (mine) q1v[0] = q1;
            q1 += cur.y; if (mine) q1v[1] = q1;
            q1 += cur.z; if (mine) q1v[2] = q1;
            q1 += cur.w; if (mine) q1v[3] = q1;
            __builtin_amdgcn_sched_barrier(0);
            cur = nxt;
        }
    }
    double q2v[4]; bool skip[4];
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = 4 * lane + k; const double q1 = q1v[k], q2 = 1. - q1; q2v[k] = q2;
        skip[k] = fmin(q1, q2) < (double)1.1920928955078125e-7f || fmax(q1, q2) > 1. - (double)1.1920928955078125e-7f;
        // the compiler's FP64 division up to the refined reciprocal (AMDGPU legalizeFDIV64: rcp, two Newton steps in FMA arithmetic)
        const double b = skip[k] ? 1.0 : q1, r0 = __builtin_amdgcn_rcp(b), e0 = fma(-b, r0, 1.0), r1 = fma(r0, e0, r0), e1 = fma(-b, r1, 1.0), y = fma(r1, e1, r1);
        s_c[i] = make_double4(q1, i * pv[k], y, skip[k] ? 1.0 : 0.0);
    }
    __syncthreads();
    double mu1v[4] = {0, 0, 0, 0};
    {   // mu1 chain: mu1 *= q1_old; then either stays (skipped bin) or becomes (mu1 + i p_i) / q1_i.  Software-pipelined by hand: the four bins of lane
        // L + 1 are fetched before the chain walks the bins of lane L (the scheduler otherwise issues each read right before its use)
        double mu1 = 0, q1_old = 0;
        double4 cur[4], nxt[4];
        #pragma unroll
        for (int k = 0; k < 4; k++) cur[k] = s_c[k];
        for (int L = 0; L < 64; L++) {
            const int Ln = min(L + 1, 63);
            #pragma unroll
            for (int k = 0; k < 4; k++) nxt[k] = s_c[4 * Ln + k];
            __builtin_amdgcn_sched_barrier(0);
            const bool mine = L == lane;
            #pragma unroll
            for (int k = 0; k < 4; k++) {
                const double4 c = cur[k];
                const double m = mu1 * q1_old, n = m + c.y, q0 = n * c.z, r = fma(-c.x, q0, n), q = fma(r, c.z, q0);
                mu1 = c.w != 0.0 ? m : q; q1_old = c.x;
                if (mine) mu1v[k] = mu1;
            }
            __builtin_amdgcn_sched_barrier(0);
            #pragma unroll
            for (int k = 0; k < 4; k++) cur[k] = nxt[k];
        }
    }
    double best = 0; int best_i = 0x7fffffff;
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = 4 * lane + k; const double mu1 = mu1v[k];
        if (dbg_mu1) dbg_mu1[i] = mu1;
        if (skip[k]) continue;
        const double q1 = q1v[k], q2 = q2v[k], mu2 = (mu - q1 * mu1) / q2, sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > best) { best = sigma; best_i = i; }
    }
    wave_argmax_f64(best, best_i);
    const double otsu_v = best > 0 ? (double)best_i : 0.0;
    // ---- Triangle
    double tri_v;
    {
        int lf = 256, rt = 0, mx = 0, mi = 0;
        #pragma unroll
        for (int k = 0; k < 4; k++) { const int i = 4 * lane + k; if (h[k] > 0) { lf = min(lf, i); if (i > 0) rt = max(rt, i); } if (h[k] > mx) { mx = h[k]; mi = i; } }
        int left = wave_min_i32(lf); if (left == 256) left = 0;
        int right = wave_max_i32(rt);
        { double mxd = mx; int mid = mx > 0 ? mi : 0x7fffffff; wave_argmax_f64(mxd, mid); mx = (int)mxd; mi = mx > 0 ? mid : 0; }
        int max_ind = mi;
        if (left > 0) left--;
        if (right < 255) right++;
        bool flipped = false;
        if (max_ind - left < right - max_ind) { flipped = true; left = 255 - right; max_ind = 255 - max_ind; }
        const double a = mx, b = left - max_ind;
        double dist = 0; int thr_i = 0x7fffffff;
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = 4 * lane + k, i = flipped ? 255 - j : j;          // position i of the (possibly mirrored) histogram holds bin j
            if (i < left + 1 || i > max_ind) continue;
            const double t = a * i + b * h[k];
            if (t > dist || (t == dist && t > 0 && i < thr_i)) { dist = t; thr_i = i; }
        }
        wave_argmax_f64(dist, thr_i);
        double thresh = dist > 0 ? (double)thr_i : (double)left;
        thresh--;
        if (flipped) thresh = 255 - thresh;
        tri_v = thresh;
    }
    // ---- clamping (wave-uniform scalars)
    float thred1 = (float)otsu_v, thred2 = (float)tri_v;
    const float otsu_f = thred1, tri_f = thred2;
    float lo, hi;
    if (thred1 < thred2) {                                    // DD:1309-1336
        if (thred1 < 1.7f * 255.0f / maxErrorf) thred1 = 1.7f * 255.0f / maxErrorf;
        else if (thred1 > 3.0f * 255.0f / maxErrorf) thred1 = 3.0f * 255.0f / maxErrorf;
        int cnt = 0;
        #pragma unroll
        for (int k = 0; k < 4; k++) if ((double)(4 * lane + k) > (double)thred1) cnt += h[k];
        cnt = wave_sum_i32(cnt);
        if (cnt > 0.5 * W * H) thred1 = thred1 + 0.2f * 255.0f / maxErrorf;
        if (thred2 < fmaxf(3.0f * 255.0f / maxErrorf, thred1 * 1.2f)) thred2 = fmaxf(3.0f * 255.0f / maxErrorf, thred1 * 1.2f);
        else if (thred2 > 10.0f * 255.0f / maxErrorf) thred2 = 10.0f * 255.0f / maxErrorf;
        lo = thred1; hi = thred2;
    } else {                                                  // DD:1337-1367 (the relaxation test there is dead code)
        if (thred2 < 1.7f * 255.0f / maxErrorf) thred2 = 1.7f * 255.0f / maxErrorf;
        else if (thred2 > 3.0f * 255.0f / maxErrorf) thred2 = 3.0f * 255.0f / maxErrorf;
        if (thred1 < fmaxf(3.0f * 255.0f / maxErrorf, thred2 * 1.2f)) thred1 = fmaxf(3.0f * 255.0f / maxErrorf, thred2 * 1.2f);
        else if (thred1 > 10.0f * 255.0f / maxErrorf) thred1 = 10.0f * 255.0f / maxErrorf;
        lo = thred2; hi = thred1;
    }
    if (lane == 0) { float* out = reinterpret_cast<float*>(res + 257); out[0] = lo; out[1] = hi; out[2] = otsu_f; out[3] = tri_f; }
    if (!keep_hist) { *reinterpret_cast<int4*>(hist + 4 * lane) = make_int4(0, 0, 0, 0); if (lane == 0) hist[256] = 0; }
}
__global__ void __launch_bounds__(64) k_flow_thresholds(int* __restrict__ hist, int W, int H, int* __restrict__ res, double* __restrict__ dbg_mu1, int keep_hist) {
    __shared__ double s_p[256];
    __shared__ double4 s_c[256];                        // per bin: q1_i, i * p_i, y_i, skip flag
    flow_thresholds_wave(hist + (size_t)blockIdx.x * 257, W, H, res + (size_t)blockIdx.x * 261, dbg_mu1 ? dbg_mu1 + (size_t)blockIdx.x * 256 : nullptr, keep_hist, s_p, s_c);
}
// one block = the histogram of one record; the result block sits behind the record's two bit masks
__global__ void __launch_bounds__(64) k_flow_thresholds_frames(const FlowMaskRec* __restrict__ recs, int W, int H, int mask_words) {
    __shared__ double s_p[256];
    __shared__ double4 s_c[256];
    const FlowMaskRec& R = recs[blockIdx.x];
    flow_thresholds_wave(R.hist, W, H, reinterpret_cast<int*>(R.out + 2 * (size_t)mask_words), nullptr, 0, s_p, s_c);
}
// both masks of every record, bit-packed in BitImg's layout (row-major, W / 64 words per row, bit x & 63 of word x >> 6): the width is a multiple of 64, so
// 64 consecutive pixels are one word and one wave ballot makes it.  Same comparison as k_threshold_masks_dev (q > (double)thr); blockIdx.y = record.
__global__ void __launch_bounds__(256) k_flow_mask_bits_frames(const FlowMaskRec* __restrict__ recs, int mask_words) {
    const FlowMaskRec& R = recs[blockIdx.y];
    const float* thr = reinterpret_cast<const float*>(reinterpret_cast<const int*>(R.out + 2 * (size_t)mask_words) + 257);
    const double tl = (double)thr[0], th = (double)thr[1];
    const int lane = threadIdx.x & 63;
    for (int word = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); word < mask_words; word += gridDim.x * (blockDim.x >> 6)) {
        const double q = (double)R.magu8[(size_t)word * 64 + lane];
        const unsigned long long lo = __ballot(q > tl), hi = __ballot(q > th);
        if (lane == 0) { R.out[word] = lo; R.out[(size_t)mask_words + word] = hi; }
    }
}
// masks from the u8 residual: low -> 128, high -> 255 (stImgMasks), thresholds read from the result block of k_flow_thresholds
// (16 pixels per thread where the planes allow 16-byte accesses: one pixel per thread was 1 200 workgroups of turnover per 640 x 480 frame).  The one-pixel-per-thread
// path is not reached from production: DynaTail, the only caller outside the debug entry, takes widths that are a multiple of 64 and heights that are a multiple of 8 and
// passes the start of allocations and a plane W * H bytes behind one, so its three planes are always 16-byte aligned.  sind_debug_flow_masks_stage runs it with a byte offset.
__global__ void k_threshold_masks_dev(const uint8_t* __restrict__ magu8, const float* __restrict__ thr, uint8_t* __restrict__ low, uint8_t* __restrict__ high, int n, int wide) {
    const double tl = (double)thr[0], th = (double)thr[1];
    if (wide) {
        const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 16;
        if (i >= n) return;
        if (i + 16 <= n) {
            const uint4 q4 = *reinterpret_cast<const uint4*>(magu8 + i);
            const unsigned qs[4] = {q4.x, q4.y, q4.z, q4.w}; unsigned lo[4], hi[4];
            #pragma unroll
            for (int k = 0; k < 4; k++) {
                lo[k] = hi[k] = 0u;
                #pragma unroll
                for (int b = 0; b < 4; b++) { const double q = (double)((qs[k] >> (8 * b)) & 255u); lo[k] |= (q > tl ? 128u : 0u) << (8 * b); hi[k] |= (q > th ? 255u : 0u) << (8 * b); }
            }
            *reinterpret_cast<uint4*>(low + i) = make_uint4(lo[0], lo[1], lo[2], lo[3]); *reinterpret_cast<uint4*>(high + i) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
            return;
        }
        for (int k = i; k < n; k++) { const double q = (double)magu8[k]; low[k] = q > tl ? 128 : 0; high[k] = q > th ? 255 : 0; }
        return;
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double q = (double)magu8[i];
    low[i] = q > tl ? 128 : 0;
    high[i] = q > th ? 255 : 0;
}

int launch_mag_stats(hipStream_t s, const float* u, const float* v, float* mag, unsigned* maxbits, int* hist, uint8_t* out_u8, int n, int B) {
    HIP_TRY(hipMemsetAsync(maxbits, 0, B * sizeof(unsigned), s));
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)B * 256 * sizeof(int), s));
    const int gx = std::min(divup(n, 256), 64);
    hipLaunchKernelGGL(k_mag_max, dim3(gx, B), dim3(256), 0, s, u, v, mag, maxbits, n);
    hipLaunchKernelGGL(k_mag_hist, dim3(gx, B), dim3(256), 0, s, mag, maxbits, hist, out_u8, n);
    return SIND_OK;
}
int launch_residual(hipStream_t s, const float* u, const float* v, const double H[9], float* mag, unsigned* maxbits, int* hist, uint8_t* magu8, int w, int h, bool already_zero) {
    HMat Hm; for (int i = 0; i < 9; i++) Hm.h[i] = H[i];
    if (already_zero) {}                                  // the consumer of the previous frame (k_flow_thresholds) left the block zeroed
    else if ((const void*)maxbits == (const void*)(hist + 256)) HIP_TRY(hipMemsetAsync(hist, 0, 257 * sizeof(int), s));       // histogram and maximum in one block: one fill
    else { HIP_TRY(hipMemsetAsync(maxbits, 0, sizeof(unsigned), s)); HIP_TRY(hipMemsetAsync(hist, 0, 256 * sizeof(int), s)); }
    hipLaunchKernelGGL(k_residual_mag, dim3(divup(w, 128), divup(h, RM_ROWS)), dim3(128), 0, s, u, v, Hm, mag, maxbits, w, h);
    const int n = w * h, gx = std::min(divup(n, 256), 64);
    hipLaunchKernelGGL(k_mag_hist, dim3(gx, 1), dim3(256), 0, s, mag, maxbits, hist, magu8, n);
    return SIND_OK;
}
int launch_flow_thresholds_and_masks(hipStream_t s, int* hist, int W, int H, int* res, const uint8_t* magu8, uint8_t* low, uint8_t* high) {
    hipLaunchKernelGGL(k_flow_thresholds, dim3(1), dim3(64), 0, s, hist, W, H, res, (double*)nullptr, 0);
    const int wide = ((((uintptr_t)magu8 | (uintptr_t)low | (uintptr_t)high) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_threshold_masks_dev, dim3(divup(wide ? divup(W * H, 16) : W * H, 256)), dim3(256), 0, s, magu8, reinterpret_cast<const float*>(res + 257), low, high, W * H, wide);
    return SIND_OK;
}
// The flow-mask stage for the n frames of a record table (device copy of `host`, which is checked here: a bad record is a wild device access) in four launches.
// Every record's working histogram must be zero on entry and is left zeroed.
int launch_flow_masks_frames(hipStream_t s, const FlowMaskRec* recs_dev, const FlowMaskRec* host, int n, int capacity, int W, int H) {
    if (n < 1 || n > capacity || !recs_dev || !host || W < 64 || W % 64 != 0 || H < 1) { sind_set_error("launch_flow_masks_frames: %d records (capacity %d), %d x %d", n, capacity, W, H); return SIND_E_ARG; }
    for (int i = 0; i < n; i++) {
        const FlowMaskRec& R = host[i];
        if (!R.U || !R.V || !R.mag || !R.magu8 || !R.hist || !R.out || ((uintptr_t)R.hist & 15) || ((uintptr_t)R.out & 15)) { sind_set_error("launch_flow_masks_frames: record %d has a null or misaligned pointer", i); return SIND_E_ARG; }
    }
    const int np = W * H, words = np / 64;
    hipLaunchKernelGGL(k_residual_mag_frames, dim3(divup(W, 128), divup(H, RM_ROWS), n), dim3(128), 0, s, recs_dev, W, H);
    hipLaunchKernelGGL(k_mag_hist_frames, dim3(std::min(divup(np, 256), 64), n), dim3(256), 0, s, recs_dev, np);
    hipLaunchKernelGGL(k_flow_thresholds_frames, dim3(n), dim3(64), 0, s, recs_dev, W, H, words);
    hipLaunchKernelGGL(k_flow_mask_bits_frames, dim3(std::min(divup(words, 16), 64), n), dim3(256), 0, s, recs_dev, words);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}
// test entry: n histograms (257 words each, device) through the one-wave kernel (variant 1; mu1 chain optionally dumped) or the serial reference (variant 0)
int debug_flow_thresholds(hipStream_t s, int* hist, int n, int W, int H, int variant, int* res, double* mu1) {
    if (variant == 0) hipLaunchKernelGGL(k_flow_thresholds_serial, dim3(n), dim3(64), 0, s, hist, W, H, reinterpret_cast<float*>(res));
    else hipLaunchKernelGGL(k_flow_thresholds, dim3(n), dim3(64), 0, s, hist, W, H, res, mu1, variant == 2 ? 0 : 1);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
