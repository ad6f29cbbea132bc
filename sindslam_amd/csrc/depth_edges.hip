// GPU front of CalOccluded and the other depth-image stencils for gfx950 (reference ORB_SLAM2/src/DynaDetect.cc):
//   CalOccluded (:429-482): medianBlur(5), 5x5 max-difference depth edge, valid-area mask
//   morphologyEx with elliptical elements (:51-59 and every MORPH_* call)
//   PEAC initial 16x16 block statistics (PEAC/AHCPlaneSeg.hpp:180-262)
//   imgDepth / depth_max * 255 -> 8U (:765-768)
// Integer stages are bit-exact; FP32 expressions are written in the reference's operation order (-ffp-contract=off).
#include "common.hpp"
#include "depth.hpp"
#include "host/peac_fit.hpp"

namespace sind {

// ---------------------------------------------------------------- medianBlur(5) on the depth image (values are integers, so the float median == u16 median)
// (the CalOccluded kernels take the frame from blockIdx.z: the pipeline runs them once for all frames of a step)
// A thread makes MED_ROWS outputs of one column: the 5 x (MED_ROWS + 4) window is loaded once (10 loads per pixel instead of 25) and a launch has a quarter of the waves.
#define MED_ROWS 4
__global__ void k_median5_u16(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int w, int h) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y0 = blockIdx.y * MED_ROWS;
    if (x >= w) return;
    src += (size_t)blockIdx.z * w * h; dst += (size_t)blockIdx.z * w * h;
    int xs[5];
    #pragma unroll
    for (int dx = -2; dx <= 2; dx++) xs[dx + 2] = min(max(x + dx, 0), w - 1);
    int win[MED_ROWS + 4][5];
    #pragma unroll
    for (int j = 0; j < MED_ROWS + 4; j++) {
        const uint16_t* r = src + (size_t)min(max(y0 - 2 + j, 0), h - 1) * w;
        #pragma unroll
        for (int k = 0; k < 5; k++) win[j][k] = r[xs[k]];
    }
    #pragma unroll
    for (int q = 0; q < MED_ROWS; q++) {
        const int y = y0 + q;
        if (y >= h) break;
        int p[25];
        #pragma unroll
        for (int j = 0; j < 5; j++) {
            #pragma unroll
            for (int k = 0; k < 5; k++) p[j * 5 + k] = win[q + j][k];
        }
        // 99 compare-exchanges instead of the 625 comparisons of a rank count (median25_net.inc)
        #define S(a, b) { const int lo_ = min(p[a], p[b]), hi_ = max(p[a], p[b]); p[a] = lo_; p[b] = hi_; }
        #include "median25_net.inc"
        #undef S
        dst[y * w + x] = (uint16_t)p[12];
    }
}
// (16-byte loads, eight samples each: with one 2-byte load per lane and turn the kernel took 0.5 ms for the 39 MB of a 64-frame round and 3 % of a step's wave cycles)
__global__ void k_max_u16(const uint16_t* __restrict__ src, int n, unsigned* __restrict__ out, int out_stride, int wide) {
    src += (size_t)blockIdx.y * n; out += (size_t)blockIdx.y * out_stride;
    unsigned m = 0;
    const int n8 = wide ? n >> 3 : 0; const uint4* s8 = reinterpret_cast<const uint4*>(src);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += gridDim.x * blockDim.x) {
        const uint4 v = s8[i];
        m = max(m, max(max(max(v.x & 0xffffu, v.x >> 16), max(v.y & 0xffffu, v.y >> 16)), max(max(v.z & 0xffffu, v.z >> 16), max(v.w & 0xffffu, v.w >> 16))));
    }
    for (int i = (n8 << 3) + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) m = max(m, (unsigned)src[i]);      // n % 8 samples at the end
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
// 5x5 max-difference depth edge + valid-area mask (DD:443-482); the 3-px frame is left 0 in both outputs
#define GE_ROWS 4
__global__ void k_grad_edge(const uint16_t* __restrict__ filt, const unsigned* __restrict__ dmax, uint8_t* __restrict__ edge,
                            uint8_t* __restrict__ total_area, int w, int h, float depthScale, int dmax_stride) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x, row0 = blockIdx.y * GE_ROWS;
    if (col >= w) return;
    { const size_t fo = (size_t)blockIdx.z * w * h; filt += fo; edge += fo; total_area += fo; dmax += (size_t)blockIdx.z * dmax_stride; }
    const bool col_in = col >= 3 && col < w - 3;
    // the 5 x (GE_ROWS + 4) window of this column's rows, loaded once (rows / columns outside the image are never used: the 3-pixel frame has no window)
    float win[GE_ROWS + 4][5];
    #pragma unroll
    for (int j = 0; j < GE_ROWS + 4; j++) {
        const int r = row0 - 2 + j; const bool in = col_in && r >= 0 && r < h;
        #pragma unroll
        for (int k = 0; k < 5; k++) win[j][k] = in ? (float)filt[r * w + col + k - 2] : 0.f;
    }
    const float depth_max = (float)(*dmax);
    #pragma unroll
    for (int q = 0; q < GE_ROWS; q++) {
        const int row = row0 + q;
        if (row >= h) break;
        uint8_t e = 0, t = 0;
        if (row >= 3 && row < h - 3 && col_in) {
            const float depth1 = win[q + 2][2];
            if (depth1 > 0.0f && depth1 / depthScale < 6.0f) t = 255;
            float val_max = 0.0f;
            #pragma unroll
            for (int i = -2; i <= 2; i++)
                #pragma unroll
                for (int j = -2; j <= 2; j++) {
                    const float nb = win[q + 2 + i][j + 2];
                    if ((depth1 - nb) > depth_max * 0.5f) continue;
                    const float a = fabsf(depth1 - nb);
                    val_max = fabsf(val_max) > a ? fabsf(val_max) : a;
                }
            if (val_max > depth1 * 0.03f && val_max > 400.0f) e = 255;
        }
        edge[row * w + col] = e; total_area[row * w + col] = t;
    }
}

// ---------------------------------------------------------------- morphology with an elliptical element (max / min over in-image pixels)
__global__ void k_morph(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, MorphElem E, int is_dilate) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    src += (size_t)blockIdx.z * w * h; dst += (size_t)blockIdx.z * w * h;
    int m = is_dilate ? 0 : 255;
    for (int i = 0; i < E.n; i++) {
        const int yy = y + i - E.ay;
        if (yy < 0 || yy >= h || E.j2[i] <= E.j1[i]) continue;
        const uint8_t* r = src + (size_t)yy * w;
        const int xa = max(x + E.j1[i] - E.ax, 0), xb = min(x + E.j2[i] - E.ax, w);
        for (int xx = xa; xx < xb; xx++) m = is_dilate ? max(m, (int)r[xx]) : min(m, (int)r[xx]);
    }
    dst[y * w + x] = (uint8_t)m;
}

// The 4 x 4 ellipse of CalOccluded's MORPH_OPEN ({(0, 0)} in the row two above, columns -2 .. +1 in the rows -1, 0, +1), a thread walking MO_ROWS rows of one column: four
// byte loads per source row serve every output row that sees it (5.5 loads per pixel instead of 13) and a launch has an eighth of the waves.  Same values as k_morph.
#define MO_ROWS 8
__global__ void k_morph_e4(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int is_dilate) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y0 = blockIdx.y * MO_ROWS;
    if (x >= w) return;
    src += (size_t)blockIdx.z * w * h; dst += (size_t)blockIdx.z * w * h;
    const int none = is_dilate ? 0 : 255;
    auto op = [&](int a, int b) { return is_dilate ? max(a, b) : min(a, b); };
    int own[MO_ROWS + 3], four[MO_ROWS + 3];                 // source row y0 - 2 + j: the pixel itself, the extreme of its columns x - 2 .. x + 1 (inside the image)
    #pragma unroll
    for (int j = 0; j < MO_ROWS + 3; j++) {
        const int yy = y0 - 2 + j;
        own[j] = none; four[j] = none;
        if (yy >= 0 && yy < h) {
            const uint8_t* r = src + (size_t)yy * w;
            const int c = r[x]; own[j] = c; int m = c;
            if (x >= 2) m = op(m, (int)r[x - 2]);
            if (x >= 1) m = op(m, (int)r[x - 1]);
            if (x + 1 < w) m = op(m, (int)r[x + 1]);
            four[j] = m;
        }
    }
    #pragma unroll
    for (int q = 0; q < MO_ROWS; q++) {
        const int y = y0 + q;
        if (y >= h) break;
        dst[y * w + x] = (uint8_t)op(op(own[q], four[q + 1]), op(four[q + 2], four[q + 3]));
    }
}
// ---------------------------------------------------------------- PEAC initial block statistics (16 x 16 blocks): one wave per SEVEN blocks.
// Phase 1, all lanes: the points of the wave's blocks (x, y, z as the FLOATS the reference forms before it widens them) and each block's validity (a block with a missing
// point or a depth jump to the right / lower neighbour is dropped as a whole, so the order of that test is free) go to LDS.  Phase 2: the nine FP64 moments of a block are
// accumulated by nine lanes, each adding its 256 terms in the reference's row-major order (bit-exact with a sequential CPU loop) -- 63 lanes = 7 blocks x 9 moments, and a term
// is two LDS reads, two conversions and one product.  (One block per wave with every term's point re-derived inside the sequential loop -- two float divisions per term on 9 of
// 64 lanes -- was 6.9 % of ALL VALU cycles of a step and 2.8 % of its CU-busy cycles: profiles/r04/pmc_by_kernel.txt.)
#define PEAC_BW 16
#define PEAC_BPW 7                                                  // blocks per wave
__global__ void __launch_bounds__(64) k_peac_block_stats(const uint16_t* __restrict__ depth, int w, int h, int Nw, int nblk, float fx, float fy, float cx, float cy,
                                                         float depthScale, double depthAlpha, double depthChangeTol, PeacBlockStats* __restrict__ out) {
    __shared__ float pt[PEAC_BPW][3][PEAC_BW * PEAC_BW];            // x, y, z per point of the wave's blocks
    const int lane = threadIdx.x, blk0 = blockIdx.x * PEAC_BPW;
    depth += (size_t)blockIdx.y * w * h; out += (size_t)blockIdx.y * nblk;
    const float inv = 1.0f / depthScale;
    auto zat = [&](int i, int j, float& zf) -> bool { const float d = (float)depth[i * w + j]; if (d < 1e-3f) return false; zf = d * inv; return true; };
    unsigned validbits = 0;                                         // wave-uniform
    for (int b = 0; b < PEAC_BPW; b++) {
        const int blk = blk0 + b;
        if (blk >= nblk) break;
        const int by = blk / Nw, bx = blk - by * Nw;
        bool ok = true;
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            const int p = k * 64 + lane, i = by * PEAC_BW + (p >> 4), j = bx * PEAC_BW + (p & 15);
            float zf = 0.f, zn;
            if (!zat(i, j, zf)) ok = false;
            else {
                const double z = (double)zf, tol = depthAlpha * fabs(z) + depthChangeTol;
                if (j + 1 < w && zat(i, j + 1, zn) && fabs(z - (double)zn) > tol) ok = false;
                if (i + 1 < h && zat(i + 1, j, zn) && fabs(z - (double)zn) > tol) ok = false;
            }
            pt[b][0][p] = (j - cx) * zf / fx; pt[b][1][p] = (i - cy) * zf / fy; pt[b][2][p] = zf;
        }
        if (__all(ok)) validbits |= 1u << b;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);                             // lgkmcnt(0): the wave's own LDS stores (wave-synchronous, no barrier needed)
    __builtin_amdgcn_wave_barrier();
    const int b = lane / 9, m = lane - 9 * b, blk = blk0 + b;
    if (b >= PEAC_BPW || blk >= nblk) return;
    const bool valid = (validbits >> b) & 1u;
    // lane (b, m) accumulates moment m of block b: sx sy sz sxx syy szz sxy syz sxz = the sums of A, or of A x B
    const int ia = (m == 1 || m == 4 || m == 7) ? 1 : (m == 2 || m == 5) ? 2 : 0, ib = (m == 3) ? 0 : (m == 4 || m == 6) ? 1 : 2;      // (x, y, z) = (0, 1, 2): xx yy zz xy yz xz
    const bool single = m < 3;
    double acc = 0;
    if (valid) {
        const float* A = pt[b][ia]; const float* B = pt[b][ib];
        #pragma unroll 4
        for (int p = 0; p < PEAC_BW * PEAC_BW; p++) {
            const double av = (double)A[p], bv = (double)B[p];
            acc += single ? av : av * bv;
        }
    }
    double* o = &out[blk].sx; o[m] = acc;
    if (m == 0) { out[blk].N = valid ? PEAC_BW * PEAC_BW : 0; out[blk].valid = valid ? 1 : 0; }
}
// Plane fit of every valid block (host/peac_fit.hpp, the host's own function): the 1200 (640 x 480) to 3600 (1280 x 720) initial nodes are a third of all the
// fits of a frame's graph clustering (~1 us each on a host core: a 3 x 3 Jacobi iteration).  One thread per block.
__global__ void k_peac_block_fit(PeacBlockStats* __restrict__ blocks, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PeacBlockStats& S = blocks[i];
    int fitted = 0;
    if (S.valid && S.N >= 4) { double c[3], nrm[3], mse; peac_fit(&S.sx, S.N, c, nrm, mse); S.mse = mse; for (int k = 0; k < 3; k++) { S.center[k] = c[k]; S.normal[k] = nrm[k]; } fitted = 1; }
    S.fitted = fitted; S.pad = 0;
}

// ---------------------------------------------------------------- imgDepth/depth_max*255 -> 8U (DD:765-768): u16 * (float)((1/max)*255), cvRound, saturate
__global__ void k_depth_norm(const uint16_t* __restrict__ depth, const unsigned* __restrict__ dmax, uint8_t* __restrict__ out, int n, int dmax_stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    depth += (size_t)blockIdx.y * n; out += (size_t)blockIdx.y * n; dmax += (size_t)blockIdx.y * dmax_stride;
    const float a = (float)((1.0 / (double)(*dmax)) * 255);
    int v = d_cvRound((float)depth[i] * a);
    v = min(max(v, 0), 65535);
    out[i] = (uint8_t)min(v, 255);
}

// ---------------------------------------------------------------- launchers
// B frames per launch (frame b at offset b * w * h of every image argument; maxima at out + b * out_stride)
int launch_median5(hipStream_t s, const uint16_t* src, uint16_t* dst, int w, int h, int B) { hipLaunchKernelGGL(k_median5_u16, dim3(divup(w, 64), divup(h, MED_ROWS), B), dim3(64), 0, s, src, dst, w, h); return SIND_OK; }
int launch_max_u16(hipStream_t s, const uint16_t* src, int n, unsigned* out, int B, int out_stride) {
    if (B == 1 || out_stride == 1) HIP_TRY(hipMemsetAsync(out, 0, (size_t)B * sizeof(unsigned), s));
    else for (int b = 0; b < B; b++) HIP_TRY(hipMemsetAsync(out + (size_t)b * out_stride, 0, sizeof(unsigned), s));
    // 16-byte loads need every image of the launch to start on a 16-byte boundary: the base pointer aligned (a per-frame pointer into a batch buffer is only when the frame
    // size is a multiple of 8 samples) and, for a batch, a multiple of 8 samples per image; anything else takes the 2-byte loop
    const int wide = ((uintptr_t)src % 16 == 0 && (B == 1 || n % 8 == 0)) ? 1 : 0;
    hipLaunchKernelGGL(k_max_u16, dim3(std::max(1, std::min(divup(n, 8 * 256), 64)), B), dim3(256), 0, s, src, n, out, out_stride, wide); return SIND_OK; }
int launch_grad_edge(hipStream_t s, const uint16_t* filt, const unsigned* dmax, uint8_t* edge, uint8_t* total_area, int w, int h, float depthScale, int B, int dmax_stride) {
    hipLaunchKernelGGL(k_grad_edge, dim3(divup(w, 128), divup(h, GE_ROWS), B), dim3(128), 0, s, filt, dmax, edge, total_area, w, h, depthScale, dmax_stride); return SIND_OK; }
MorphElem make_ellipse(int n) {
    MorphElem e; e.n = n; e.ax = n / 2; e.ay = n / 2;
    for (int i = 0; i < MORPH_MAX; i++) { e.j1[i] = 0; e.j2[i] = 0; }
    if (n == 1) { e.j2[0] = 1; return e; }
    const int r = n / 2, c = n / 2; const double inv_r2 = r ? 1. / ((double)r * r) : 0;
    for (int i = 0; i < n; i++) {
        const int dy = i - r;
        if (std::abs(dy) <= r) { const int dx = (int)std::lrint(c * std::sqrt((r * r - dy * dy) * inv_r2)); e.j1[i] = std::max(c - dx, 0); e.j2[i] = std::min(c + dx + 1, n); }
    }
    return e;
}
int launch_morph(hipStream_t s, const uint8_t* src, uint8_t* dst, int w, int h, int n, bool dilate, int B) {
    if (n == 4) { hipLaunchKernelGGL(k_morph_e4, dim3(divup(w, 128), divup(h, MO_ROWS), B), dim3(128), 0, s, src, dst, w, h, dilate ? 1 : 0); return SIND_OK; }
    hipLaunchKernelGGL(k_morph, dim3(divup(w, 128), h, B), dim3(128), 0, s, src, dst, w, h, make_ellipse(n), dilate ? 1 : 0); return SIND_OK; }
int launch_peac_block_stats(hipStream_t s, const uint16_t* depth, int w, int h, int bw, int bh, float fx, float fy, float cx, float cy, float depthScale, PeacBlockStats* out, int B) {
    if (bw != PEAC_BW || bh != PEAC_BW) { sind_set_error("peac_block_stats: %d x %d blocks (only %d x %d)", bw, bh, PEAC_BW, PEAC_BW); return SIND_E_ARG; }
    const int nb = (w / bw) * (h / bh);
    hipLaunchKernelGGL(k_peac_block_stats, dim3(divup(nb, PEAC_BPW), B), dim3(64), 0, s, depth, w, h, w / bw, nb, fx, fy, cx, cy, depthScale, 0.04, 0.02 * 1000, out);
    hipLaunchKernelGGL(k_peac_block_fit, dim3(divup(nb * B, 64)), dim3(64), 0, s, out, nb * B); return SIND_OK; }
int launch_depth_norm(hipStream_t s, const uint16_t* depth, const unsigned* dmax, uint8_t* out, int n, int B, int dmax_stride) {
    hipLaunchKernelGGL(k_depth_norm, dim3(divup(n, 256), B), dim3(256), 0, s, depth, dmax, out, n, dmax_stride); return SIND_OK; }

}  // namespace sind
