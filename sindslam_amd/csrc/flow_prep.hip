// Dense variational optical flow for DynaDetect on gfx950 (CDNA4): batched DeepFlow (variational part) and
// VariationalRefinement, i.e. the path reference DynaDetect.cc:1031-1147 spends ~99 % of its bytes in
// (SURVEY.md §8 a-3..a-7).  Every kernel is batched over B frame pairs: planes are laid out [B][h][w] in HBM,
// blockIdx.z (or .y for 1-D kernels) is the pair index, consecutive lanes walk consecutive x (coalesced rows).
// One kernel family per file: this one prepares the images (conversion, blur, resizing, the 0.95 pyramid, the frame-history pool, the sample grid);
// flow_level.hip is a pyramid level around its solver, flow_sor.hip chooses and launches the solver (kernels there and in flow_stream.hip, flow_wave.hip,
// flow_coarse.hip), flow_mask.hip is the flow-mask stage.
//
// Arithmetic contract: built with -ffp-contract=off and IEEE divide/sqrt so that every FP32 expression below is
// evaluated exactly like OpenCV's scalar code paths (variational_refinement.cpp, deepflow.cpp, resize.cpp,
// imgwarp.cpp remap); the parity tests compare these kernels with the CPU oracle bit for bit.
//
// Roofline: all kernels here are HBM/L2-bound stencil passes (no MFMA: nothing is a contraction).
#include "flow_dev.hpp"

namespace sind {

// ---------------------------------------------------------------------------------------------------------
// u8 -> f32 (+ optional 3x3 Gaussian, BORDER_REFLECT_101): deepflow.cpp pre-smoothing with sigma = 0.6.
// Separable form kept (row pass value T, then column pass over T) so rounding matches sepFilter2D.
__global__ void k_u8_to_f32_blur3(const uint8_t* __restrict__ src, float* __restrict__ dst, int w, int h, float k0, float k1, int do_blur) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= w) return;
    const uint8_t* S = src + (size_t)b * w * h;
    float* D = dst + (size_t)b * w * h;
    if (!do_blur) { D[y * w + x] = (float)S[y * w + x]; return; }
    const int xl = d_reflect101(x - 1, w), xr = d_reflect101(x + 1, w);
    const int yu = d_reflect101(y - 1, h), yd = d_reflect101(y + 1, h);
    auto rowv = [&](int yy) { const uint8_t* r = S + yy * w; return (float)r[x] * k0 + ((float)r[xl] + (float)r[xr]) * k1; };
    const float U = rowv(yu), C = rowv(y), L = rowv(yd);
    D[y * w + x] = C * k0 + (U + L) * k1;
}

// ---------------------------------------------------------------------------------------------------------
// cv::resize(INTER_LINEAR) on CV_32F (resize.cpp): used for the 0.95 pyramid, the flow up-sampling between
// levels (post = 1/0.95) and the final 384x288 -> 640x480 up-scale (post = 1/0.6).  scale_* are doubles computed
// on the host exactly as OpenCV does (1 / ((double)dsize/ssize)).
// Two batches with the same geometry in one launch (both images of the pairs for the pyramid, both flow components for the up-sampling): blockIdx.z =
// image + B * (0 | 1).
// A thread makes RZ_ROWS destination pixels of one column: the horizontal weights are formed once, and a launch has a quarter of the workgroups (one pixel per thread was
// bound by workgroup dispatch: 294 k workgroups of 128 threads for the top level of 170 pairs, 131 us for 0.3 GB).  The per-pixel expressions are resize_px's.
#define RZ_ROWS 4
__global__ void k_resize_f32_pair(const float* __restrict__ srcA, float* __restrict__ dstA, const float* __restrict__ srcB, float* __restrict__ dstB, int B,
                                  int sw, int sh, int dw, int dh, double scale_x, double scale_y, float post, int has_post) {
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy0 = blockIdx.y * RZ_ROWS; int b = blockIdx.z;
    if (dx >= dw) return;
    const float* src = srcA; float* dst = dstA;
    if (b >= B) { b -= B; src = srcB; dst = dstB; }
    const float* S = src + (size_t)b * sw * sh; float* D = dst + (size_t)b * dw * dh;
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = d_cvFloorf(fx); fx -= sx;
    const bool two = sx + 1 < sw;            // dx < xmax in OpenCV's HResizeLinear
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    const float a1 = fx, a0 = 1.f - a1;
    #pragma unroll
    for (int r = 0; r < RZ_ROWS; r++) {
        const int dy = dy0 + r;
        if (dy >= dh) break;
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = d_cvFloorf(fy); fy -= sy;
        const int y0 = d_clip(sy, 0, sh), y1 = d_clip(sy + 1, 0, sh);
        const float b1 = fy, b0 = 1.f - b1;
        const float* R0 = S + (size_t)y0 * sw; const float* R1 = S + (size_t)y1 * sw;
        float r0, r1;
        if (two) { r0 = R0[sx] * a0 + R0[sx + 1] * a1; r1 = R1[sx] * a0 + R1[sx + 1] * a1; }
        else     { r0 = R0[sx] * 1.f;                  r1 = R1[sx] * 1.f; }
        float v = r0 * b0 + r1 * b1;
        if (has_post) v = v * post;
        D[(size_t)dy * dw + dx] = v;
    }
}
// The small levels of the 0.95 pyramid in ONE launch: a workgroup walks levels first+1 .. first+n of one image (level l from level l-1, a barrier in
// between; the image is <= 12 k pixels there) instead of one launch per level and image -- the chain of ~2 x 27 dependent launches per slice sat at the
// start of every step, when nothing else of the step can run yet.
#define PYR_TAIL_MAX 40
struct PyrTail { int n, B; int w[PYR_TAIL_MAX + 1], h[PYR_TAIL_MAX + 1]; unsigned long long off[PYR_TAIL_MAX + 1]; double sx[PYR_TAIL_MAX + 1], sy[PYR_TAIL_MAX + 1]; };
__global__ void __launch_bounds__(256) k_pyramid_tail(float* __restrict__ pyrA, float* __restrict__ pyrB, PyrTail T) {
    int b = blockIdx.x; float* pyr = pyrA;
    if (b >= T.B) { b -= T.B; pyr = pyrB; }
    for (int k = 1; k <= T.n; k++) {
        const int sw = T.w[k - 1], sh = T.h[k - 1], dw = T.w[k], dh = T.h[k];
        const float* S = pyr + T.off[k - 1] + (size_t)b * sw * sh; float* D = pyr + T.off[k] + (size_t)b * dw * dh;
        for (int i = threadIdx.x; i < dw * dh; i += 256) { const int dy = i / dw, dx = i - dy * dw; D[i] = resize_px(S, sw, sh, dx, dy, T.sx[k], T.sy[k]); }
        __syncthreads();                     // level k complete (and visible to the workgroup) before level k + 1 reads it
    }
}
__global__ void k_resize_f32(const float* __restrict__ src, float* __restrict__ dst, int sw, int sh, int dw, int dh,
                             double scale_x, double scale_y, float post, int has_post) {
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y, b = blockIdx.z;
    if (dx >= dw) return;
    const float* S = src + (size_t)b * sw * sh;
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = d_cvFloorf(fx); fx -= sx;
    const bool two = sx + 1 < sw;            // dx < xmax in OpenCV's HResizeLinear
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    int sy = d_cvFloorf(fy); fy -= sy;
    const int y0 = d_clip(sy, 0, sh), y1 = d_clip(sy + 1, 0, sh);
    const float a1 = fx, a0 = 1.f - a1, b1 = fy, b0 = 1.f - b1;
    const float* R0 = S + (size_t)y0 * sw; const float* R1 = S + (size_t)y1 * sw;
    float r0, r1;
    if (two) { r0 = R0[sx] * a0 + R0[sx + 1] * a1; r1 = R1[sx] * a0 + R1[sx + 1] * a1; }
    else     { r0 = R0[sx] * 1.f;                  r1 = R1[sx] * 1.f; }
    float v = r0 * b0 + r1 * b1;
    if (has_post) v = v * post;
    dst[(size_t)b * dw * dh + (size_t)dy * dw + dx] = v;
}

// ---------------------------------------------------------------------------------------------------------
// cvtColor(BGR2GRAY) 8U fixed point and cv::resize(INTER_LINEAR) 8U (11-bit coefficients), reference DD:1390-1392, 1037-1039
__global__ void k_bgr2gray(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ gray, size_t n, int cb, int cr) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = bgr + i * 3;
    gray[i] = (uint8_t)((p[0] * cb + p[1] * 9617 + p[2] * cr + 8192) >> 14);
}
// four pixels per thread: three 4-byte loads, one 4-byte store (n4 = whole quads; needs 4-byte aligned images)
__global__ void k_bgr2gray4(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ gray, size_t n4, int cb, int cr) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const unsigned* p = reinterpret_cast<const unsigned*>(bgr) + i * 3;
    const unsigned a = p[0], b = p[1], c = p[2];             // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
    auto g = [&](unsigned bb, unsigned gg, unsigned rr) { return (unsigned)(((int)bb * cb + (int)gg * 9617 + (int)rr * cr + 8192) >> 14) & 0xffu; };
    const unsigned g0 = g(a & 0xff, (a >> 8) & 0xff, (a >> 16) & 0xff), g1 = g(a >> 24, b & 0xff, (b >> 8) & 0xff);
    const unsigned g2 = g((b >> 16) & 0xff, b >> 24, c & 0xff), g3 = g((c >> 8) & 0xff, (c >> 16) & 0xff, c >> 24);
    reinterpret_cast<unsigned*>(gray)[i] = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
}
__global__ void k_resize_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int sw, int sh, int dw, int dh,
                            double scale_x, double scale_y, int s_stride, int d_stride, size_t s_img, size_t d_img, int d_group, int d_skip) {
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy0 = blockIdx.y * RZ_ROWS, b = blockIdx.z;      // RZ_ROWS destination rows of a column per thread, like k_resize_f32_pair
    if (dx >= dw) return;
    const uint8_t* S = src + (size_t)b * s_img;
    const int db = d_group > 0 ? b + (b / d_group) * d_skip : b;       // destination slot: groups of d_group images, d_skip slots left free after each group
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = d_cvFloorf(fx); fx -= sx;
    const bool two = sx + 1 < sw;
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    const int ax0 = (short)d_cvRound((1.f - fx) * 2048), ax1 = (short)d_cvRound(fx * 2048);
    #pragma unroll
    for (int r = 0; r < RZ_ROWS; r++) {
        const int dy = dy0 + r;
        if (dy >= dh) break;
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = d_cvFloorf(fy); fy -= sy;
        const int y0 = d_clip(sy, 0, sh), y1 = d_clip(sy + 1, 0, sh);
        const int b0 = (short)d_cvRound((1.f - fy) * 2048), b1 = (short)d_cvRound(fy * 2048);
        const uint8_t* R0 = S + (size_t)y0 * s_stride; const uint8_t* R1 = S + (size_t)y1 * s_stride;
        int r0, r1;
        if (two) { r0 = R0[sx] * ax0 + R0[sx + 1] * ax1; r1 = R1[sx] * ax0 + R1[sx + 1] * ax1; }
        else     { r0 = R0[sx] * 2048;                   r1 = R1[sx] * 2048; }
        dst[(size_t)db * d_img + (size_t)dy * d_stride + dx] = (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
    }
}

// frames of the gray history pool picked by index into a dense batch: out[b] = pool[idx[b]] (16 bytes per thread; the indices travel as
// kernel arguments, up to 256 per launch) -- one launch instead of one device-to-device copy per frame (3 000 copies per 512-pair step)
struct GatherIdx { int v[256]; };
// End of a step: the last two flow-grid frames of every stream become its history slots 0, 1 (the pool holds T + 2 slots per stream).  One thread moves the
// same 16 bytes of both frames and reads before it writes, so T = 1 (slot 1 is source and destination) needs no second buffer.
__global__ void k_roll_history(uint8_t* __restrict__ pool, int T, size_t fb16) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= fb16) return;
    uint4* base = reinterpret_cast<uint4*>(pool) + (size_t)blockIdx.y * (T + 2) * fb16;
    const uint4 a = base[(size_t)T * fb16 + i], b = base[(size_t)(T + 1) * fb16 + i];
    base[i] = a; base[fb16 + i] = b;
}
__global__ void k_gather_frames(const uint8_t* __restrict__ pool, GatherIdx idx, uint8_t* __restrict__ out, size_t fb) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (i >= fb) return;
    const uint8_t* s = pool + (size_t)idx.v[blockIdx.y] * fb + i; uint8_t* d = out + (size_t)blockIdx.y * fb + i;
    if (i + 16 <= fb) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
    else for (size_t k = 0; i + k < fb; k++) d[k] = s[k];
}

// gather flow at the 63x47 sample grid (DD:1182-1204) so the host can build the PROSAC-ordered pairs
__global__ void k_gather_grid(const float* __restrict__ u, const float* __restrict__ v, float* __restrict__ out, int w, int h, int step) {
    const int gx = (w - 1) / step, gy = (h - 1) / step;   // points at step, 2*step, ... < w
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;      // blockIdx.y = frame of a batch (dense [B][h][w] planes)
    if (i >= gx * gy) return;
    const int r = (i / gx + 1) * step, c = (i % gx + 1) * step;
    const size_t fo = (size_t)b * w * h;
    out[((size_t)b * gx * gy + i) * 2] = u[fo + r * w + c]; out[((size_t)b * gx * gy + i) * 2 + 1] = v[fo + r * w + c];
}

__global__ void k_scale(float* __restrict__ a, float* __restrict__ b, float s, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a[i] = a[i] * s; b[i] = b[i] * s;
}

// ---------------------------------------------------------------------------------------------------------
// host-side launchers
static inline dim3 grid2d(int w, int h, int B, int bx = 128) { return dim3(divup(w, bx), h, B); }

int launch_gather_frames(hipStream_t s, const uint8_t* pool, const int* idx_host, int B, uint8_t* out, size_t fb) {
    if (fb % 16 != 0) { sind_set_error("launch_gather_frames: frame size %zu is not a multiple of 16 bytes", fb); return SIND_E_ARG; }
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int nb = std::min(256, B - b0); GatherIdx a;
        for (int i = 0; i < nb; i++) a.v[i] = idx_host[b0 + i];
        hipLaunchKernelGGL(k_gather_frames, dim3((unsigned)((fb / 16 + 255) / 256), nb), dim3(256), 0, s, pool, a, out + (size_t)b0 * fb, fb);
    }
    return SIND_OK;
}
int launch_u8_to_f32_blur3(hipStream_t s, const uint8_t* src, float* dst, int w, int h, int B, float k0, float k1, bool blur) {
    hipLaunchKernelGGL(k_u8_to_f32_blur3, grid2d(w, h, B), dim3(128), 0, s, src, dst, w, h, k0, k1, blur ? 1 : 0);
    return SIND_OK;
}
int launch_resize_f32(hipStream_t s, const float* src, float* dst, int sw, int sh, int dw, int dh, int B, float post, bool has_post) {
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    hipLaunchKernelGGL(k_resize_f32, grid2d(dw, dh, B), dim3(128), 0, s, src, dst, sw, sh, dw, dh, scale_x, scale_y, post, has_post ? 1 : 0);
    return SIND_OK;
}
int launch_resize_f32_pair(hipStream_t s, const float* srcA, float* dstA, const float* srcB, float* dstB, int sw, int sh, int dw, int dh, int B, float post, bool has_post) {
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    hipLaunchKernelGGL(k_resize_f32_pair, grid2d(dw, divup(dh, RZ_ROWS), 2 * B), dim3(128), 0, s, srcA, dstA, srcB, dstB, B, sw, sh, dw, dh, scale_x, scale_y, post, has_post ? 1 : 0);
    return SIND_OK;
}
// levels first+1 .. last of both pyramids (level l of image b at pyr + off[l] * B + b * w[l] * h[l]) from level `first`, which must be complete
int launch_pyramid_tail(hipStream_t s, float* pyrA, float* pyrB, const std::vector<std::pair<int, int>>& levels, const std::vector<size_t>& level_off, int first, int last, int B) {
    if (last <= first) return SIND_OK;
    if (last - first > PYR_TAIL_MAX) { sind_set_error("launch_pyramid_tail: %d levels (at most %d)", last - first, PYR_TAIL_MAX); return SIND_E_ARG; }
    PyrTail T; T.n = last - first; T.B = B;
    for (int k = 0; k <= T.n; k++) {
        const int l = first + k; T.w[k] = levels[l].first; T.h[k] = levels[l].second; T.off[k] = (unsigned long long)level_off[l] * B;
        if (k > 0) { T.sx[k] = 1. / ((double)T.w[k] / T.w[k - 1]); T.sy[k] = 1. / ((double)T.h[k] / T.h[k - 1]); } else { T.sx[k] = T.sy[k] = 1; }
    }
    hipLaunchKernelGGL(k_pyramid_tail, dim3(2 * B), dim3(256), 0, s, pyrA, pyrB, T);
    return SIND_OK;
}
int launch_roll_history(hipStream_t s, uint8_t* pool, int S, int T, size_t frame_bytes) {
    if (frame_bytes % 16) { sind_set_error("roll_history: frame size %zu is not a multiple of 16", frame_bytes); return SIND_E_ARG; }
    const size_t fb16 = frame_bytes / 16;
    hipLaunchKernelGGL(k_roll_history, dim3((unsigned)((fb16 + 255) / 256), S), dim3(256), 0, s, pool, T, fb16);
    return SIND_OK;
}
int launch_resize_u8(hipStream_t s, const uint8_t* src, uint8_t* dst, int sw, int sh, int dw, int dh, int B, int s_stride, int d_stride, size_t s_img, size_t d_img, int d_group, int d_skip) {
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    hipLaunchKernelGGL(k_resize_u8, grid2d(dw, divup(dh, RZ_ROWS), B), dim3(128), 0, s, src, dst, sw, sh, dw, dh, scale_x, scale_y, s_stride, d_stride, s_img, d_img, d_group, d_skip);
    return SIND_OK;
}
int launch_bgr2gray(hipStream_t s, const uint8_t* bgr, uint8_t* gray, size_t npix, bool swap_rb) {
    if ((npix & 3) == 0 && (((uintptr_t)bgr | (uintptr_t)gray) & 3) == 0)
        hipLaunchKernelGGL(k_bgr2gray4, dim3((unsigned)((npix / 4 + 255) / 256)), dim3(256), 0, s, bgr, gray, npix / 4, swap_rb ? 4899 : 1868, swap_rb ? 1868 : 4899);
    else
        hipLaunchKernelGGL(k_bgr2gray, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, bgr, gray, npix, swap_rb ? 4899 : 1868, swap_rb ? 1868 : 4899);
    return SIND_OK;
}
int launch_gather_grid(hipStream_t s, const float* u, const float* v, float* out, int w, int h, int step, int B) {
    const int cnt = ((w - 1) / step) * ((h - 1) / step);
    hipLaunchKernelGGL(k_gather_grid, dim3(divup(cnt, 256), B), dim3(256), 0, s, u, v, out, w, h, step);
    return SIND_OK;
}
int launch_scale2(hipStream_t s, float* a, float* b, float sc, size_t n) {
    hipLaunchKernelGGL(k_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, sc, n);
    return SIND_OK;
}

}  // namespace sind
