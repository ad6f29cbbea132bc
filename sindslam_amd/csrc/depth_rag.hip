// SegAndMergeV2 region-adjacency statistics for gfx950 (reference ORB_SLAM2/src/DynaDetect.cc :784-893, cal_hist :1685-1739) from per-pixel
// membership words, and the 7 x 7 dilation of the pieces' bit planes ahead of them.  Integer counts: bit-exact.
#include <mutex>
#include "common.hpp"
#include "depth.hpp"

namespace sind {

// ---------------------------------------------------------------- region-adjacency statistics (SegAndMergeV2 RAG build + cal_hist inputs)
// Input: bit planes [3][C][h*wpr] (img = piece mask, dil = 7-dilated piece, lj = "lianjie" fake-edge mask), 64 px per word.
// Each lane takes one pixel; the 64 lanes of a wavefront share the plane words (broadcast loads) and assemble the pixel's
// membership words.  One pass produces overlap[i][j] = |dil_i & dil_j|, overlapPlane[i][j] = |dil_i & dil_j & occ2|,
// ljOverlap[i][j], ljArea[i] and hist[i][v] = 256-bin histogram of the normalised depth over img_i (value 255 dropped:
// calcHist ranges {0,255}).  Counters are privatised in LDS when they fit (C <= 64) and flushed once per workgroup.
// (body shared by the per-frame kernel and the frame-indexed one: the three plane sets as pointers of their own, the workgroup's index and count among
// those of its frame, and the LDS block)
template <bool USE_LDS>
__device__ __forceinline__ void rag_stats_body(const unsigned long long* __restrict__ p_img, const unsigned long long* __restrict__ p_dil, const unsigned long long* __restrict__ p_lj,
                                               int C, int w, int h, int wpr, const uint8_t* __restrict__ occ2, const uint8_t* __restrict__ depthN,
                                               int* __restrict__ overlap, int* __restrict__ overlapPlane, int* __restrict__ ljOverlap,
                                               int* __restrict__ ljArea, int* __restrict__ hist, int* sm, int block, int nblocks) {
    int *lh = hist, *lo = overlap, *lp = overlapPlane, *ll = ljOverlap, *la = ljArea;
    if (USE_LDS) {
        lh = sm; lo = lh + C * 256; lp = lo + C * C; ll = lp + C * C; la = ll + C * C;
        const int total = C * 256 + 3 * C * C + C;
        for (int i = threadIdx.x; i < total; i += 256) sm[i] = 0;
        __syncthreads();
    }
    const int NW = (C + 63) >> 6;
    const size_t pw = (size_t)h * wpr;           // words per plane
    const int n = w * h;
    for (int i = block * 256 + threadIdx.x; i < n; i += nblocks * 256) {
        const int y = i / w, x = i - y * w; const size_t widx = (size_t)y * wpr + (x >> 6); const int bit = x & 63;
        // The 64 lanes of a wave sit on the 64 pixels of ONE plane word (w % 64 == 0 and every stride is a multiple of 64): lane c fetches
        // the three words of piece c once, and each lane then picks its own bit out of the words broadcast with readlane -- 3 loads per
        // 64 pieces instead of 3*C dependent loads per pixel, which is what this kernel's time used to be.
        unsigned long long mi[4] = {0, 0, 0, 0}, md[4] = {0, 0, 0, 0}, ml[4] = {0, 0, 0, 0};
        const int lane = threadIdx.x & 63;
        #pragma unroll
        for (int q = 0; q < 4; q++) {
            if (q >= NW) break;
            const int c = (q << 6) + lane;
            unsigned long long wi = 0, wd = 0, wl = 0;
            if (c < C) { wi = p_img[(size_t)c * pw + widx]; wd = p_dil[(size_t)c * pw + widx]; wl = p_lj[(size_t)c * pw + widx]; }
            const int cnt = min(64, C - (q << 6));
            // lane `bit` wants bit `bit` of piece cc's words as bit cc of its own: the half of the word the lane's pixel lies in is fixed per lane, the half of the result per cc --
            // 32-bit operations throughout (three instead of six per plane and piece: the 64-bit shifts by a lane-varying and by a uniform count were two passes each)
            const bool upper = bit >= 32; const unsigned sh = (unsigned)bit & 31u;
            unsigned ri[2] = {0u, 0u}, rd[2] = {0u, 0u}, rl[2] = {0u, 0u};
            #pragma unroll
            for (int hh = 0; hh < 2; hh++) {
                const int c0 = hh * 32, c1 = min(cnt, c0 + 32);
                for (int cc = c0; cc < c1; cc++) {
                    const unsigned alo = (unsigned)__builtin_amdgcn_readlane((int)wi, cc), ahi = (unsigned)__builtin_amdgcn_readlane((int)(wi >> 32), cc);
                    const unsigned dlo = (unsigned)__builtin_amdgcn_readlane((int)wd, cc), dhi = (unsigned)__builtin_amdgcn_readlane((int)(wd >> 32), cc);
                    const unsigned llo = (unsigned)__builtin_amdgcn_readlane((int)wl, cc), lhi = (unsigned)__builtin_amdgcn_readlane((int)(wl >> 32), cc);
                    const unsigned k = (unsigned)(cc - c0);
                    ri[hh] |= (((upper ? ahi : alo) >> sh) & 1u) << k; rd[hh] |= (((upper ? dhi : dlo) >> sh) & 1u) << k; rl[hh] |= (((upper ? lhi : llo) >> sh) & 1u) << k;
                }
            }
            mi[q] = ((unsigned long long)ri[1] << 32) | ri[0]; md[q] = ((unsigned long long)rd[1] << 32) | rd[0]; ml[q] = ((unsigned long long)rl[1] << 32) | rl[0];
        }
        const int dv = depthN[i];
        if (dv < 255) {
            #pragma unroll
            for (int q = 0; q < 4; q++) { if (q >= NW) break; unsigned long long m = mi[q]; while (m) { const int c = (q << 6) + __ffsll((long long)m) - 1; m &= m - 1; atomicAdd(&lh[c * 256 + dv], 1); } }
        }
        int nd = 0, nl = 0;
        #pragma unroll
        for (int q = 0; q < 4; q++) { nd += __popcll(md[q]); nl += __popcll(ml[q]); }
        if (nd >= 2) {
            const bool pl = occ2[i] != 0;
            for (int ci = 0; ci < C; ci++) { if (!((md[ci >> 6] >> (ci & 63)) & 1ull)) continue;
                for (int cj = ci + 1; cj < C; cj++) { if (!((md[cj >> 6] >> (cj & 63)) & 1ull)) continue; atomicAdd(&lo[ci * C + cj], 1); if (pl) atomicAdd(&lp[ci * C + cj], 1); } }
        }
        if (nl >= 1) {
            for (int ci = 0; ci < C; ci++) { if (!((ml[ci >> 6] >> (ci & 63)) & 1ull)) continue; atomicAdd(&la[ci], 1);
                for (int cj = ci + 1; cj < C; cj++) { if (!((ml[cj >> 6] >> (cj & 63)) & 1ull)) continue; atomicAdd(&ll[ci * C + cj], 1); } }
        }
    }
    if (USE_LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < C * 256; i += 256) if (lh[i]) atomicAdd(&hist[i], lh[i]);
        for (int i = threadIdx.x; i < C * C; i += 256) { if (lo[i]) atomicAdd(&overlap[i], lo[i]); if (lp[i]) atomicAdd(&overlapPlane[i], lp[i]); if (ll[i]) atomicAdd(&ljOverlap[i], ll[i]); }
        for (int i = threadIdx.x; i < C; i += 256) if (la[i]) atomicAdd(&ljArea[i], la[i]);
    }
}
template <bool USE_LDS>
__global__ void __launch_bounds__(256) k_rag_stats(const unsigned long long* __restrict__ planes, int C, int w, int h, int wpr,
                                                   const uint8_t* __restrict__ occ2, const uint8_t* __restrict__ depthN,
                                                   int* __restrict__ overlap, int* __restrict__ overlapPlane, int* __restrict__ ljOverlap,
                                                   int* __restrict__ ljArea, int* __restrict__ hist) {
    extern __shared__ int sm[];
    const size_t pw = (size_t)h * wpr;
    rag_stats_body<USE_LDS>(planes, planes + (size_t)C * pw, planes + (size_t)2 * C * pw, C, w, h, wpr, occ2, depthN, overlap, overlapPlane, ljOverlap, ljArea, hist, sm, blockIdx.x, gridDim.x);
}
// One frame of every stream of a k-means group: blockIdx.y = the frame's record (depth.hpp), blockIdx.x = one of the few workgroups of that frame -- the
// parallelism comes from the frames, so a frame's counters are zeroed and flushed by 8 - 32 workgroups instead of 128.  The launch's dynamic LDS holds the counters
// of the chunk's largest C <= 64; a frame with more pieces counts in global memory (uniform per workgroup).  Counts are integers: any partition gives the same numbers.
__global__ void __launch_bounds__(256) k_rag_stats_frames(const RagRec* __restrict__ recs, const unsigned long long* __restrict__ in, const unsigned long long* __restrict__ dil,
                                                          int* __restrict__ res, int w, int h, int wpr) {
    extern __shared__ int sm[];
    const RagRec R = recs[blockIdx.y];
    const int C = R.C; const size_t pw = (size_t)h * wpr;
    const unsigned long long* p_img = in + R.plane_off; const unsigned long long* p_lj = p_img + (size_t)C * pw; const unsigned long long* p_dil = dil + R.plane_off / 2;
    int* ov = res + R.res_off; int* ovp = ov + C * C; int* lj = ovp + C * C; int* la = lj + C * C; int* hs = la + C;
    if (C <= 64) rag_stats_body<true>(p_img, p_dil, p_lj, C, w, h, wpr, R.occ2, R.depthN, ov, ovp, lj, la, hs, sm, blockIdx.x, gridDim.x);
    else rag_stats_body<false>(p_img, p_dil, p_lj, C, w, h, wpr, R.occ2, R.depthN, ov, ovp, lj, la, hs, sm, blockIdx.x, gridDim.x);
}

// Elliptical dilation of bit planes (64 pixels per word), dst(x, y) = OR over the element of src(x + j - ax, y + i - ay) with positions
// outside the image ignored: the 7x7 dilation of every piece of SegAndMergeV2 (DD:760-ish "imgEachClusterDilate") for the region-adjacency
// statistics.  One thread per output word; a row of the element is a run of <= 15 shifts over a three-word window.
// zero / nzero (optional): a block of ints cleared on the way -- the accumulators of k_rag_stats, which follows on the same stream (one fill launch less per frame).
__device__ __forceinline__ unsigned long long dilate_plane_word(const unsigned long long* __restrict__ sp, int y, int k, int wpr, int H, const MorphElem& e, unsigned long long tail_mask) {
    unsigned long long acc = 0ull;
    for (int i = 0; i < e.n; i++) {
        const int ys = y + i - e.ay;
        if (ys < 0 || ys >= H || e.j2[i] <= e.j1[i]) continue;
        const unsigned long long* r = sp + (size_t)ys * wpr;
        const unsigned long long cur = r[k], prev = k > 0 ? r[k - 1] : 0ull, next = k + 1 < wpr ? r[k + 1] : 0ull;
        for (int j = e.j1[i]; j < e.j2[i]; j++) {
            const int t = j - e.ax;                      // dst bit x takes src bit x + t
            if (t == 0) acc |= cur;
            else if (t > 0) acc |= (cur >> t) | (next << (64 - t));
            else acc |= (cur << (-t)) | (prev >> (64 + t));
        }
    }
    if (k == wpr - 1) acc &= tail_mask;
    return acc;
}
__global__ void k_dilate_planes(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, int nplanes, int wpr, int H, MorphElem e,
                                unsigned long long tail_mask, int* __restrict__ zero, int nzero) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, pw = (size_t)wpr * H;
    for (size_t z = idx; z < (size_t)nzero; z += (size_t)gridDim.x * blockDim.x) zero[z] = 0;
    if (idx >= pw * nplanes) return;
    const int c = (int)(idx / pw), rem = (int)(idx - (size_t)c * pw), y = rem / wpr, k = rem - y * wpr;
    dst[idx] = dilate_plane_word(src + (size_t)c * pw, y, k, wpr, H, e, tail_mask);
}
// the same for one frame of every stream of a group: blockIdx.y = the frame's record, the grid's x extent covers the chunk's largest C; every frame's
// result block is cleared on the way
__global__ void k_dilate_planes_frames(const RagRec* __restrict__ recs, const unsigned long long* __restrict__ in, unsigned long long* __restrict__ dil, int* __restrict__ res,
                                       int wpr, int H, MorphElem e, unsigned long long tail_mask) {
    const RagRec R = recs[blockIdx.y];
    const int C = R.C;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, pw = (size_t)wpr * H;
    const size_t nzero = (size_t)3 * C * C + C + (size_t)C * 256;
    int* zero = res + R.res_off;
    for (size_t z = idx; z < nzero; z += (size_t)gridDim.x * blockDim.x) zero[z] = 0;
    if (idx >= pw * C) return;
    const int c = (int)(idx / pw), rem = (int)(idx - (size_t)c * pw), y = rem / wpr, k = rem - y * wpr;
    dil[R.plane_off / 2 + idx] = dilate_plane_word(in + R.plane_off + (size_t)c * pw, y, k, wpr, H, e, tail_mask);
}
int launch_dilate_planes(hipStream_t s, const unsigned long long* src, unsigned long long* dst, int nplanes, int w, int h, int n, int* zero, int nzero) {
    const int wpr = (w + 63) / 64; const size_t total = (size_t)wpr * h * nplanes;
    const unsigned long long tm = (w & 63) ? ((1ull << (w & 63)) - 1) : ~0ull;
    hipLaunchKernelGGL(k_dilate_planes, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, nplanes, wpr, h, make_ellipse(n), tm, zero, zero ? nzero : 0);
    return SIND_OK;
}

// ---------------------------------------------------------------- launchers
int launch_rag_stats(hipStream_t s, const unsigned long long* planes, int C, int w, int h, int wpr, const uint8_t* occ2, const uint8_t* depthN,
                     int* overlap, int* overlapPlane, int* ljOverlap, int* ljArea, int* hist, bool already_zero) {
    if (C < 1 || C > 254) { sind_set_error("rag_stats: %d pieces unsupported (1..254)", C); return SIND_E_ARG; }
    if (already_zero) {}                                  // cleared by the dilation kernel ahead of this one on the stream
    else if (overlapPlane == overlap + C * C && ljOverlap == overlapPlane + C * C && ljArea == ljOverlap + C * C && hist == ljArea + C)
        HIP_TRY(hipMemsetAsync(overlap, 0, ((size_t)3 * C * C + C + (size_t)C * 256) * sizeof(int), s));        // the caller's five outputs are one block: one fill
    else {
        HIP_TRY(hipMemsetAsync(overlap, 0, (size_t)C * C * sizeof(int), s)); HIP_TRY(hipMemsetAsync(overlapPlane, 0, (size_t)C * C * sizeof(int), s));
        HIP_TRY(hipMemsetAsync(ljOverlap, 0, (size_t)C * C * sizeof(int), s)); HIP_TRY(hipMemsetAsync(ljArea, 0, (size_t)C * sizeof(int), s));
        HIP_TRY(hipMemsetAsync(hist, 0, (size_t)C * 256 * sizeof(int), s));
    }
    if (C <= 64) {
        const size_t shm = ((size_t)C * 256 + 3 * (size_t)C * C + C) * sizeof(int);      // <= 64 KB + 48 KB + 256 B of the 160 KB LDS
        static SindPerDeviceInit attr_init;       // the pool's workers call this concurrently; once per device
        HIP_TRY(attr_init.run([] { return hipFuncSetAttribute((const void*)k_rag_stats<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024); }));
        hipLaunchKernelGGL(k_rag_stats<true>, dim3(128), dim3(256), shm, s, planes, C, w, h, wpr, occ2, depthN, overlap, overlapPlane, ljOverlap, ljArea, hist);
    } else {
        hipLaunchKernelGGL(k_rag_stats<false>, dim3(256), dim3(256), 0, s, planes, C, w, h, wpr, occ2, depthN, overlap, overlapPlane, ljOverlap, ljArea, hist);
    }
    return SIND_OK;
}
int launch_rag_frames(hipStream_t s, const RagRec* recs_dev, const RagRec* host, int n, const unsigned long long* in, size_t in_words, unsigned long long* dil, int* res, size_t res_ints, int w, int h) {
    if (n < 1 || n > 65535 || !recs_dev || !host || !in || !dil || !res || w < 64 || w % 64 != 0 || h < 1) { sind_set_error("launch_rag_frames: %d records, %d x %d", n, w, h); return SIND_E_ARG; }
    const int wpr = w / 64; const size_t pw = (size_t)h * wpr;
    int maxC = 0, maxLds = 0;
    for (int i = 0; i < n; i++) {
        const RagRec& R = host[i];
        if (R.C < 1 || R.C > 254 || !R.occ2 || !R.depthN || (R.plane_off & 1) || R.plane_off + (size_t)2 * R.C * pw > in_words || R.res_off + rag_result_ints(R.C) > res_ints) {
            sind_set_error("launch_rag_frames: record %d (%d pieces) has a null pointer or leaves its slab", i, R.C); return SIND_E_ARG; }
        maxC = std::max(maxC, R.C); if (R.C <= 64) maxLds = std::max(maxLds, R.C);
    }
    hipLaunchKernelGGL(k_dilate_planes_frames, dim3((unsigned)((pw * maxC + 255) / 256), n), dim3(256), 0, s, recs_dev, in, dil, res, wpr, h, make_ellipse(7), ~0ull);
    // workgroups per frame: the frame's counters (C = 20: 6 340) are zeroed and flushed once per workgroup, each of which should have many more pixels than that --
    // 8 at 64 frames (150 pixels per thread at 640 x 480), up to 32 for a small chunk, no more than the frame has 256-pixel groups
    const int per_frame = std::max(1, std::min(std::max(8, std::min(32, 512 / n)), (int)((size_t)w * h / 256)));
    const size_t shm = rag_result_ints(maxLds) * sizeof(int);
    static SindPerDeviceInit attr_init;
    HIP_TRY(attr_init.run([] { return hipFuncSetAttribute((const void*)k_rag_stats_frames, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024); }));
    hipLaunchKernelGGL(k_rag_stats_frames, dim3(per_frame, n), dim3(256), shm, s, recs_dev, in, dil, res, w, h, wpr);
    return SIND_OK;
}

}  // namespace sind
