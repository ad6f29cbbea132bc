// One pyramid level of the variational flow around its solver: warp, the coefficient kernels, W += dW, the level transition, varref_level; and the scans
// that check the short division and square-root forms of flow_dev.hpp against the IEEE ones.  (The solver: flow_sor.hip.)
#include "flow_dev.hpp"

namespace sind {

// ---------------------------------------------------------------------------------------------------------
// VariationalRefinementImpl::prepareBuffers, part 1: warp I1 by the level's initial flow (cv::remap, INTER_LINEAR,
// BORDER_REPLICATE, coordinates quantised to 1/32 px), averaged image and temporal difference.
#define WARP_ROWS 4                                             // rows of its column a thread makes (a quarter of the waves; the per-pixel expressions are unchanged)
__global__ void k_warp_avg_iz(const float* __restrict__ I0, const float* __restrict__ I1, const float* __restrict__ Wu,
                              const float* __restrict__ Wv, float* __restrict__ avg, float* __restrict__ Iz, float* __restrict__ dWu,
                              float* __restrict__ dWv, int w, int h) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, yb = blockIdx.y * WARP_ROWS, b = blockIdx.z;
    if (x >= w) return;
    const size_t base = (size_t)b * w * h;
    const float* S = I1 + base;
    #pragma unroll
    for (int r = 0; r < WARP_ROWS; r++) {
        const int y = yb + r;
        if (y >= h) break;
        const int i = y * w + x;
        dWu[base + i] = 0.f; dWv[base + i] = 0.f;           // the level's flow increment starts at zero (two fills less per level)
        warp_px(S, I0[base + i], Wu[base + i], Wv[base + i], x, y, w, h, avg[base + i], Iz[base + i]);
    }
}

// ---------------------------------------------------------------------------------------------------------
// One fixed-point iteration set-up: ComputeDataTerm + ComputeSmoothnessTerm{Hor,Vert}Pass gathered per pixel.
// The four smoothness contributions are added in the order OpenCV's red/black passes produce for the pixel's colour.
// A thread walks KC_ROWS consecutive rows of its column: the smoothness weight of a pixel is also its right neighbour's "left" weight and its lower
// neighbour's "upper" weight, so the left one comes from the neighbouring lane (wave shuffle; the first lane of a wave computes it) and the upper one
// from the thread's previous row (the first row of a block computes it) -- 1.3 instead of 3 weight evaluations (two loads rows, a square root and a
// division each) per pixel, same values bit for bit.
#define KC_ROWS 4
// IN: every pixel this wave touches in these rows -- the four rows of its 64 columns and their stencils (two columns / rows to every side) -- lies inside the image: no index is
// clamped and no border case exists, so every neighbour is a load at a CONSTANT offset from one of a few row pointers.  (The clamped form spends ~3 integer VALU instructions on
// each of its 49 loads per pixel: ~150 of the kernel's 376 VALU instructions per pixel, disassembly of round 4; the interior is > 95 % of a 384 x 288 level.)  Same loads of the
// same values, same arithmetic: bit-identical by construction (tests/test_flow_gpu.py).
template <bool IN>
__device__ __forceinline__ void kc_rows(const VarParams& P, int w, int h, int x, int y0, size_t base, const float* __restrict__ gAvg, const float* __restrict__ gIz, const float* __restrict__ gWu,
                       const float* __restrict__ gWv,
                       const float* __restrict__ gdWu, const float* __restrict__ gdWv, float* __restrict__ A11, float* __restrict__ A12,
                       float* __restrict__ A22, float* __restrict__ B1, float* __restrict__ B2, float* __restrict__ Wgt) {
    const float zeta2 = P.zeta * P.zeta, eps2 = P.epsilon * P.epsilon, gamma2 = P.gamma / 2, delta2 = P.delta / 2, alpha2 = P.alpha / 2;
    // The seven Sobel(ksize = 1, BORDER_REPLICATE) derivative images of prepareBuffers are formed here from the warped average and
    // the temporal difference (the float operations k_derivs used to store, evaluated at the same replicated positions): two planes
    // are read through the cache instead of eight from memory, in each of the five fixed-point iterations of a level.
    const float* A = gAvg + base; const float* Z = gIz + base;
    auto cx = [&](int v) { return IN ? v : min(max(v, 0), w - 1); };
    auto cy = [&](int v) { return IN ? v : min(max(v, 0), h - 1); };
    auto dX = [&](const float* Pp, int yy, int xx) { return Pp[yy * w + cx(xx + 1)] - Pp[yy * w + cx(xx - 1)]; };
    auto dY = [&](const float* Pp, int yy, int xx) { return Pp[cy(yy + 1) * w + xx] - Pp[cy(yy - 1) * w + xx]; };
    // tempW = W + dW is formed on the fly (OpenCV keeps it in a buffer that it refreshes after every fixed-point iteration with this
    // very addition): two planes less to read here and no k_add_flow pass between the iterations.  Before the first iteration
    // dW = 0, and W + 0 differs from W only in the sign of a zero, which the squared differences below cannot see.
    const float* WU = gWu + base; const float* WV = gWv + base; const float* DU = gdWu + base; const float* DV = gdWv + base;
    auto wgt_at = [&](int yy, int xx) {
        const int xn = IN ? xx + 1 : min(xx + 1, w - 1), yn = IN ? yy + 1 : min(yy + 1, h - 1);
        const int ic = yy * w + xx, ix = yy * w + xn, iy = yn * w + xx;
        const float c_u = WU[ic] + DU[ic], c_v = WV[ic] + DV[ic];
        const float ux = (WU[ix] + DU[ix]) - c_u, vx = (WV[ix] + DV[ix]) - c_v;
        const float uy = (WU[iy] + DU[iy]) - c_u, vy = (WV[iy] + DV[iy]) - c_v;
        return alpha2 / sqrtf(ux * ux + vx * vx + uy * uy + vy * vy + eps2);
    };
    const bool wave_first = (threadIdx.x & 63) == 0;
    float w_up = 0.f;                                       // weight of (y - 1, x): computed for the block's first row, carried down afterwards
    #pragma unroll
    for (int r = 0; r < KC_ROWS; r++) {
        const int y = y0 + r;
        if (!IN && y >= h) break;                           // uniform over the block
        const int i = y * w + x;
        const float Ix = dX(A, y, x), Iy = dY(A, y, x), Iz = Z[i], Ixz = dX(Z, y, x), Iyz = dY(Z, y, x);
        const float Ixx = dX(A, y, cx(x + 1)) - dX(A, y, cx(x - 1));
        const float Ixy = dX(A, cy(y + 1), x) - dX(A, cy(y - 1), x);
        const float Iyy = dY(A, cy(y + 1), x) - dY(A, cy(y - 1), x);
        const float dU = gdWu[base + i], dV = gdWv[base + i];
        float derivNorm = Ix * Ix + Iy * Iy + zeta2;
        const float Ik1z = Iz + Ix * dU + Iy * dV;
        const float rN0 = kc_rcp(derivNorm);
        float weight = kc_div(delta2 / sqrtf(kc_div(Ik1z * Ik1z, derivNorm, rN0) + eps2), derivNorm, rN0);
        float a11 = weight * (Ix * Ix) + zeta2;
        float a12 = weight * (Ix * Iy);
        float a22 = weight * (Iy * Iy) + zeta2;
        float b1 = -weight * (Iz * Ix);
        float b2 = -weight * (Iz * Iy);
        derivNorm = Ixx * Ixx + Ixy * Ixy + zeta2;
        const float derivNorm2 = Iyy * Iyy + Ixy * Ixy + zeta2;
        const float Ik1zx = Ixz + Ixx * dU + Ixy * dV;
        const float Ik1zy = Iyz + Ixy * dU + Iyy * dV;
        const float rN1 = kc_rcp(derivNorm), rN2 = kc_rcp(derivNorm2);
        #define D1(n) kc_div((n), derivNorm, rN1)
        #define D2(n) kc_div((n), derivNorm2, rN2)
        weight = gamma2 / sqrtf(D1(Ik1zx * Ik1zx) + D2(Ik1zy * Ik1zy) + eps2);
        a11 += weight * (D1(Ixx * Ixx) + D2(Ixy * Ixy));
        a12 += weight * (D1(Ixx * Ixy) + D2(Ixy * Iyy));
        a22 += weight * (D1(Ixy * Ixy) + D2(Iyy * Iyy));
        b1 += -weight * (D1(Ixx * Ixz) + D2(Ixy * Iyz));
        b2 += -weight * (D1(Ixy * Ixz) + D2(Iyy * Iyz));
        #undef D1
        #undef D2

        const float wp = wgt_at(y, x);
        const float w_from_lane = __shfl_up(wp, 1);          // the left neighbour's own weight (same row, lane - 1)
        const float wl = (IN || x > 0) ? (wave_first ? wgt_at(y, x - 1) : w_from_lane) : 0.f;
        const float wq = (IN || y > 0) ? (r == 0 ? wgt_at(y - 1, x) : w_up) : 0.f;
        const float wu_c = WU[i], wv_c = WV[i];
        const bool red = ((x + y) & 1) == 0;
        // the four link updates (no-ops at the image border)
        #define OWN_H() if (IN || x < w - 1) { b1 += wp * (WU[i + 1] - wu_c); a11 += wp; b2 += wp * (WV[i + 1] - wv_c); a22 += wp; }
        #define LEFT_H() if (IN || x > 0) { b1 -= wl * (wu_c - WU[i - 1]); a11 += wl; b2 -= wl * (wv_c - WV[i - 1]); a22 += wl; }
        #define OWN_V() if (IN || y < h - 1) { b1 += wp * (WU[i + w] - wu_c); a11 += wp; b2 += wp * (WV[i + w] - wv_c); a22 += wp; }
        #define UP_V() if (IN || y > 0) { b1 -= wq * (wu_c - WU[i - w]); a11 += wq; b2 -= wq * (wv_c - WV[i - w]); a22 += wq; }
        if (red) { OWN_H() LEFT_H() OWN_V() UP_V() }
        else     { LEFT_H() OWN_H() UP_V() OWN_V() }
        #undef OWN_H
        #undef LEFT_H
        #undef OWN_V
        #undef UP_V
        A11[base + i] = a11; A12[base + i] = a12; A22[base + i] = a22; B1[base + i] = b1; B2[base + i] = b2; Wgt[base + i] = wp;
        w_up = wp;
    }
}
__global__ void k_coef(VarParams P, int w, int h, const float* __restrict__ gAvg, const float* __restrict__ gIz, const float* __restrict__ gWu,
                       const float* __restrict__ gWv,
                       const float* __restrict__ gdWu, const float* __restrict__ gdWv, float* __restrict__ A11, float* __restrict__ A12,
                       float* __restrict__ A22, float* __restrict__ B1, float* __restrict__ B2, float* __restrict__ Wgt) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.z, y0 = blockIdx.y * KC_ROWS;
    if (x >= w) return;
    const size_t base = (size_t)b * w * h;
    // interior: rows y0 - 2 .. y0 + KC_ROWS + 1 and, for every lane of the wave, columns x - 2 .. x + 2 exist (wave-uniform: a ballot over the wave's live lanes)
    const bool in = y0 >= 2 && y0 + KC_ROWS + 1 < h && __builtin_amdgcn_ballot_w64(x < 2 || x + 2 >= w) == 0ull;
    if (in) kc_rows<true>(P, w, h, x, y0, base, gAvg, gIz, gWu, gWv, gdWu, gdWv, A11, A12, A22, B1, B2, Wgt);
    else kc_rows<false>(P, w, h, x, y0, base, gAvg, gIz, gWu, gWv, gdWu, gdWv, A11, A12, A22, B1, B2, Wgt);
}
// grid (tiles of KL_COLS columns, groups of 4 x KL_ROWS rows, pairs), 256 threads: wave k of a workgroup takes the rows (4 * blockIdx.y + k) * KL_ROWS ...
__global__ __launch_bounds__(256) void k_coef_lanes(VarParams P, int w, int h, const float* __restrict__ gAvg, const float* __restrict__ gIz, const float* __restrict__ gWu,
                       const float* __restrict__ gWv, const float* __restrict__ gdWu, const float* __restrict__ gdWv, float* __restrict__ A11, float* __restrict__ A12,
                       float* __restrict__ A22, float* __restrict__ B1, float* __restrict__ B2, float* __restrict__ Wgt, int fast_math,
                       int tiles_x, int tiles_y, int n_tiles, int xcd) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // 1-D grid (a multiple of 8): tile = x + tiles_x * (y + tiles_y * pair).  xcd: consecutive tiles -- the tiles of one pair, which share their halo rows and columns -- go to the
    // SAME XCD (workgroups are handed to the eight XCDs round-robin), so the second reader of a halo line finds it in that XCD's L2
    const int tile = xcd ? ((int)blockIdx.x & 7) * ((int)gridDim.x >> 3) + ((int)blockIdx.x >> 3) : (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const int bx = tile % tiles_x, byz = tile / tiles_x, by = byz % tiles_y, bz = byz / tiles_y;
    const int c0 = bx * KL_COLS - 2, y0 = (by * 4 + wave) * KL_ROWS;
    if (y0 >= h) return;                                    // whole wave
    const size_t base = (size_t)bz * w * h;
    const int col = c0 + lane;
    const bool store_lane = lane >= 2 && lane < 2 + KL_COLS && col < w;
    // the short forms of sqrt and c / sqrt need arguments >= 2^-96: every argument carries epsilon^2 (1e-6 with the reference's parameters); any other epsilon takes the IEEE forms
    const bool interior = c0 >= 0 && c0 + 63 < w && y0 >= 2 && y0 + KL_ROWS + 1 < h, fastm = P.epsilon >= 1e-12f && fast_math != 0;
    if (fastm) {
        if (interior) kc_lanes<false, true>(P, w, h, col, y0, base, gAvg, gIz, gWu, gWv, gdWu, gdWv, A11, A12, A22, B1, B2, Wgt, store_lane);
        else kc_lanes<true, true>(P, w, h, col, y0, base, gAvg, gIz, gWu, gWv, gdWu, gdWv, A11, A12, A22, B1, B2, Wgt, store_lane);
    } else {
        if (interior) kc_lanes<false, false>(P, w, h, col, y0, base, gAvg, gIz, gWu, gWv, gdWu, gdWv, A11, A12, A22, B1, B2, Wgt, store_lane);
        else kc_lanes<true, false>(P, w, h, col, y0, base, gAvg, gIz, gWu, gWv, gdWu, gdWv, A11, A12, A22, B1, B2, Wgt, store_lane);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Level transition of the DeepFlow loop in ONE launch instead of three (k_add_flow, k_resize_f32_pair, k_warp_avg_iz of the next level; deepflow.cpp: W += dW; resize(W) / 0.95;
// prepareBuffers of the next level).  A thread makes LU_ROWS pixels of one column of the NEXT level: the up-sampled flow from the four taps of fl(W + dW) -- the very values
// k_add_flow would have stored --, times `post`; then the warp of I1 by that flow, the averaged image and the temporal difference; and the next level's zero increment, which goes
// to the ping-pong partner of dW (other threads still read this level's dW as taps).  Same float operations on the same values as the three kernels: same bits.
#define LU_ROWS 4
__global__ void k_level_up(const float* __restrict__ Wu, const float* __restrict__ Wv, const float* __restrict__ dWu, const float* __restrict__ dWv, int sw, int sh,
                           const float* __restrict__ I0, const float* __restrict__ I1, float* __restrict__ nWu, float* __restrict__ nWv, float* __restrict__ ndWu, float* __restrict__ ndWv,
                           float* __restrict__ avg, float* __restrict__ Iz, int dw, int dh, double scale_x, double scale_y, float post) {
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy0 = blockIdx.y * LU_ROWS, b = blockIdx.z;
    if (dx >= dw) return;
    const size_t sbase = (size_t)b * sw * sh, dbase = (size_t)b * dw * dh;
    const float* SU = Wu + sbase; const float* SV = Wv + sbase; const float* DU = dWu + sbase; const float* DV = dWv + sbase;
    const float* S1 = I1 + dbase;
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = d_cvFloorf(fx); fx -= sx;
    const bool two = sx + 1 < sw;            // dx < xmax in OpenCV's HResizeLinear
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    const float a1 = fx, a0 = 1.f - a1;
    #pragma unroll
    for (int r = 0; r < LU_ROWS; r++) {
        const int dy = dy0 + r;
        if (dy >= dh) break;
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = d_cvFloorf(fy); fy -= sy;
        const int y0 = d_clip(sy, 0, sh), y1 = d_clip(sy + 1, 0, sh);
        const float b1 = fy, b0 = 1.f - b1;
        const int i00 = y0 * sw + sx, i10 = y1 * sw + sx;
        float ru0, ru1, rv0, rv1;
        if (two) {
            ru0 = (SU[i00] + DU[i00]) * a0 + (SU[i00 + 1] + DU[i00 + 1]) * a1; ru1 = (SU[i10] + DU[i10]) * a0 + (SU[i10 + 1] + DU[i10 + 1]) * a1;
            rv0 = (SV[i00] + DV[i00]) * a0 + (SV[i00 + 1] + DV[i00 + 1]) * a1; rv1 = (SV[i10] + DV[i10]) * a0 + (SV[i10 + 1] + DV[i10 + 1]) * a1;
        } else {
            ru0 = (SU[i00] + DU[i00]) * 1.f; ru1 = (SU[i10] + DU[i10]) * 1.f; rv0 = (SV[i00] + DV[i00]) * 1.f; rv1 = (SV[i10] + DV[i10]) * 1.f;
        }
        float vu = ru0 * b0 + ru1 * b1, vv = rv0 * b0 + rv1 * b1;
        vu = vu * post; vv = vv * post;
        const size_t o = dbase + (size_t)dy * dw + dx;
        nWu[o] = vu; nWv[o] = vv; ndWu[o] = 0.f; ndWv[o] = 0.f;
        warp_px(S1, I0[o], vu, vv, dx, dy, dw, dh, avg[o], Iz[o]);
    }
}
// after the call the planes of P describe the next level: W = the up-sampled flow, dW = 0, avg / Iz = its warped buffers
int launch_level_up(hipStream_t s, FlowPlanes& P, int sw, int sh, const float* I0, const float* I1, int dw, int dh, int B, float post) {
    hipLaunchKernelGGL(k_level_up, dim3(divup(dw, 128), divup(dh, LU_ROWS), B), dim3(128), 0, s, P.Wu, P.Wv, P.dWu, P.dWv, sw, sh, I0, I1, P.tWu, P.tWv, P.dWu2, P.dWv2, P.avg, P.Iz, dw, dh,
                       1. / ((double)dw / sw), 1. / ((double)dh / sh), post);
    HIP_TRY(hipGetLastError());
    std::swap(P.Wu, P.tWu); std::swap(P.Wv, P.tWv); std::swap(P.dWu, P.dWu2); std::swap(P.dWv, P.dWv2);
    return SIND_OK;
}

// four elements per thread (16-byte accesses; `n4` whole quads, the n % 4 elements behind them by the last threads)
__global__ void k_add_flow(const float* Wu, const float* Wv, const float* __restrict__ dWu,
                           const float* __restrict__ dWv, float* tWu, float* tWv, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n4 = n >> 2;
    if (i < n4) {
        const float4 a = reinterpret_cast<const float4*>(Wu)[i], b = reinterpret_cast<const float4*>(dWu)[i], c = reinterpret_cast<const float4*>(Wv)[i], d = reinterpret_cast<const float4*>(dWv)[i];
        reinterpret_cast<float4*>(tWu)[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        reinterpret_cast<float4*>(tWv)[i] = make_float4(c.x + d.x, c.y + d.y, c.z + d.z, c.w + d.w);
    } else {
        const size_t k = (n4 << 2) + (i - n4);
        if (k < n) { tWu[k] = Wu[k] + dWu[k]; tWv[k] = Wv[k] + dWv[k]; }
    }
}
__global__ void k_add_flow_1(const float* Wu, const float* Wv, const float* __restrict__ dWu,
                             const float* __restrict__ dWv, float* tWu, float* tWv, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tWu[i] = Wu[i] + dWu[i]; tWv[i] = Wv[i] + dWv[i];
}

__global__ void k_debug_rcp_scan(int exp_lo, int exp_hi, unsigned long long* __restrict__ out) {
    const unsigned m = blockIdx.x * blockDim.x + threadIdx.x;           // all 2^23 significands
    if (m >= (1u << 23)) return;
    unsigned long long bad_r = 0, bad_q = 0; unsigned rng = m * 2654435761u + 12345u;
    for (int e = exp_lo; e <= exp_hi; e++) {
        const float a = __uint_as_float(((unsigned)(127 + e) << 23) | m);
        const float y = sor_rcp(a), ref = 1.f / a;
        if (__float_as_uint(y) != __float_as_uint(ref)) bad_r++;
        for (int k = 0; k < 8; k++) {                                   // quotients through the reciprocal (Markstein) against the IEEE division
            rng = rng * 1664525u + 1013904223u;
            const float n = __uint_as_float((rng & 0x807fffffu) | ((unsigned)(127 + e - 40 + (int)(((rng >> 23) & 127) % 81)) << 23));
            const float q = sor_div(n, a, y), qr = n / a;
            if (__float_as_uint(q) != __float_as_uint(qr)) bad_q++;
            const float q2 = sor_div(n, -a, -y), qr2 = n / -a;
            if (__float_as_uint(q2) != __float_as_uint(qr2)) bad_q++;
        }
    }
    if (bad_r) atomicAdd(&out[0], bad_r);
    if (bad_q) atomicAdd(&out[1], bad_q);
    if (bad_r) atomicMin(&out[2], (unsigned long long)m);
}
// kc_sqrt against sqrtf, and c / b through kc_rcp + kc_div against the IEEE division for three numerators, for every significand and the binary exponents exp_lo .. exp_hi
__global__ void k_debug_coef_math_scan(int exp_lo, int exp_hi, float n0, float n1, float n2, unsigned long long* __restrict__ out) {
    const unsigned m = blockIdx.x * blockDim.x + threadIdx.x;           // all 2^23 significands
    if (m >= (1u << 23)) return;
    unsigned long long bad_s = 0, bad_q = 0;
    for (int e = exp_lo; e <= exp_hi; e++) {
        const float x = __uint_as_float(((unsigned)(127 + e) << 23) | m);
        if (__float_as_uint(kc_sqrt(x)) != __float_as_uint(sqrtf(x))) bad_s++;
        const float r = kc_rcp(x);
        if (__float_as_uint(kc_div(n0, x, r)) != __float_as_uint(n0 / x)) bad_q++;
        if (__float_as_uint(kc_div(n1, x, r)) != __float_as_uint(n1 / x)) bad_q++;
        if (__float_as_uint(kc_div(n2, x, r)) != __float_as_uint(n2 / x)) bad_q++;
    }
    if (bad_s) atomicAdd(&out[0], bad_s);
    if (bad_q) atomicAdd(&out[1], bad_q);
}
// sor_div and kc_div against the IEEE division BELOW the quotients of the two scans above: every divisor significand x the divisor exponents -7 .. 14 (the data term's and
// the solver's diagonals) x one numerator of random sign and significand per binary exponent from -149 (the smallest denormal) up to the divisor's exponent - 40, then +0 and -0.
// out[0] / out[1] = quotients of sor_div / kc_div that differ, out[2] = those among them whose numerator is a zero, out[3] = 200 + the largest numerator exponent of a
// mismatch (0: none), out[4 + 149 + e] = mismatches at the numerator exponent e (both helpers)
#define DIV_SCAN_EA_LO (-7)
#define DIV_SCAN_EA_HI 14
__global__ void __launch_bounds__(256) k_debug_div_scan(unsigned long long* __restrict__ out) {
    __shared__ unsigned by_exp[160];
    for (int i = threadIdx.x; i < 160; i += blockDim.x) by_exp[i] = 0;
    __syncthreads();
    const unsigned m = blockIdx.x * blockDim.x + threadIdx.x;           // all 2^23 significands
    unsigned long long bad_s = 0, bad_k = 0, bad_z = 0; unsigned rng = m * 2654435761u + 977u;
    for (int en = -149; en <= DIV_SCAN_EA_HI - 40; en++) {
        unsigned bad = 0;
        for (int ea = max(DIV_SCAN_EA_LO, en + 40); ea <= DIV_SCAN_EA_HI; ea++) {
            const float a = __uint_as_float(((unsigned)(127 + ea) << 23) | m);
            rng = rng * 1664525u + 1013904223u;
            const unsigned mag = en >= -126 ? (((unsigned)(127 + en) << 23) | ((rng >> 8) & 0x7fffffu)) : ((1u << (en + 149)) | ((rng >> 8) & ((1u << (en + 149)) - 1u)));
            const float n = __uint_as_float(mag | (rng & 0x80000000u)), ref = n / a;
            if (__float_as_uint(sor_div(n, a, sor_rcp(a))) != __float_as_uint(ref)) { bad_s++; bad++; }
            if (__float_as_uint(kc_div(n, a, kc_rcp(a))) != __float_as_uint(ref)) { bad_k++; bad++; }
        }
        if (bad) atomicAdd(&by_exp[en + 149], bad);
    }
    for (int ea = DIV_SCAN_EA_LO; ea <= DIV_SCAN_EA_HI; ea++) {
        const float a = __uint_as_float(((unsigned)(127 + ea) << 23) | m);
        for (unsigned z = 0; z < 2; z++) {
            const float n = __uint_as_float(z << 31), ref = n / a;
            if (__float_as_uint(sor_div(n, a, sor_rcp(a))) != __float_as_uint(ref)) { bad_s++; bad_z++; }
            if (__float_as_uint(kc_div(n, a, kc_rcp(a))) != __float_as_uint(ref)) { bad_k++; bad_z++; }
        }
    }
    if (bad_s) atomicAdd(&out[0], bad_s);
    if (bad_k) atomicAdd(&out[1], bad_k);
    if (bad_z) atomicAdd(&out[2], bad_z);
    __syncthreads();
    for (int i = threadIdx.x; i < 160; i += blockDim.x) if (by_exp[i]) { atomicAdd(&out[4 + i], (unsigned long long)by_exp[i]); atomicMax(&out[3], (unsigned long long)(200 + i - 149)); }
}
int debug_div_scan(hipStream_t s, unsigned long long* out_dev) {
    hipLaunchKernelGGL(k_debug_div_scan, dim3((1u << 23) / 256), dim3(256), 0, s, out_dev);
    HIP_TRY(hipGetLastError()); return SIND_OK;
}
int debug_coef_math_scan(hipStream_t s, int exp_lo, int exp_hi, const float numer[3], unsigned long long* out_dev) {
    hipLaunchKernelGGL(k_debug_coef_math_scan, dim3((1u << 23) / 256), dim3(256), 0, s, exp_lo, exp_hi, numer[0], numer[1], numer[2], out_dev);
    HIP_TRY(hipGetLastError()); return SIND_OK;
}
int debug_rcp_scan(hipStream_t s, int exp_lo, int exp_hi, unsigned long long* out_dev) {
    hipLaunchKernelGGL(k_debug_rcp_scan, dim3((1u << 23) / 256), dim3(256), 0, s, exp_lo, exp_hi, out_dev);
    HIP_TRY(hipGetLastError()); return SIND_OK;
}

// VariationalRefinement::calcUV on one pyramid level for B pairs.  Wu/Wv: initial flow in, refined flow out.
int varref_level(hipStream_t s, FlowPlanes& P, const float* I0, const float* I1, int w, int h, int B, const VarParams& V, SorTimer* timer, const SolverCfg& C, bool have_buffers, bool leave_increment) {
    SorPlan plan;
    SIND_TRY(sor_plan(w, h, B, V.sorIterations, V.epsilon, C, &plan));
    if (plan.kernel == SOR_COARSE_CHAIN) {       // one workgroup's work: the whole level in one launch (flow_coarse.hip)
        const std::vector<std::pair<int, int>> lv{{w, h}}; const std::vector<size_t> off{0};
        return launch_coarse_chain(s, P, I0, I1, lv, off, 0, 0, B, V, false, false, 1.f, nullptr, nullptr);
    }
    const size_t n = (size_t)w * h * B;
    const dim3 blk(128);
    // have_buffers: the level transition (k_level_up) has left avg / Iz and a zero increment already; leave_increment: W += dW is the next transition's business
    if (!have_buffers) hipLaunchKernelGGL(k_warp_avg_iz, dim3(divup(w, 128), divup(h, WARP_ROWS), B), blk, 0, s, I0, I1, P.Wu, P.Wv, P.avg, P.Iz, P.dWu, P.dWv, w, h);
    for (int it = 0; it < V.fixedPointIterations; it++) {
        if (C.coef_kernel) {
            const int tx = divup(w, KL_COLS), ty = divup(h, 4 * KL_ROWS), nt = tx * ty * B;
            hipLaunchKernelGGL(k_coef_lanes, dim3(divup(nt, 8) * 8), dim3(256), 0, s, V, w, h, P.avg, P.Iz, P.Wu, P.Wv,
                               P.dWu, P.dWv, P.A11, P.A12, P.A22, P.b1, P.b2, P.wgt, C.coef_kernel == 2 ? 0 : 1, tx, ty, nt, C.coef_xcd);
        }
        else
            hipLaunchKernelGGL(k_coef, dim3(divup(w, 128), divup(h, KC_ROWS), B), blk, 0, s, V, w, h, P.avg, P.Iz, P.Wu, P.Wv,
                               P.dWu, P.dWv, P.A11, P.A12, P.A22, P.b1, P.b2, P.wgt);
        if (timer) timer->begin(s);
        long long nlaunch = 0;
        SIND_TRY(sor_iterations(s, P, w, h, B, V.omega, plan, C, &nlaunch));
        // algorithmic bytes: 44 B per pixel per red+black iteration (9 reads + 2 writes of f32), SURVEY.md §8d
        if (timer) timer->end(s, nlaunch, 44.0 * (double)w * h * B * V.sorIterations, sor_timer_kind(plan.kernel));
    }
    if (leave_increment) { HIP_TRY(hipGetLastError()); return SIND_OK; }
    if ((((uintptr_t)P.Wu | (uintptr_t)P.Wv | (uintptr_t)P.dWu | (uintptr_t)P.dWv) & 15) == 0)
        hipLaunchKernelGGL(k_add_flow, dim3((unsigned)(((n >> 2) + (n & 3) + 255) / 256)), dim3(256), 0, s, P.Wu, P.Wv, P.dWu, P.dWv, P.Wu, P.Wv, n);      // W = W + dW, in place
    else
        hipLaunchKernelGGL(k_add_flow_1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P.Wu, P.Wv, P.dWu, P.dWv, P.Wu, P.Wv, n);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
