// SegAndMerge piece extraction for gfx950, first stage: the external borders of bit planes (reference DynaDetect.cc:675, cv::findContours RETR_EXTERNAL CHAIN_APPROX_NONE),
// bit for bit what find_contours(external_only) of host/contours.hpp returns.  One wave per plane.  The walk around a border is the host's own state machine
// (trace_border, one source for both sides), run by lane 0 on 2-bit cells: it is exact by construction.  The raster scan between two borders is the wave's: nothing
// happens inside a run of equal cells, so the 64 lanes compare 1024 cells with the value the scan carries and a ballot names the first one that differs.
// Capacities and bounds: pieces_dev.hpp.
#include "pieces_dev.hpp"
#include "host/contours.hpp"

namespace sind {

// cells: 0 background, 1 set and unmarked, 2 marked, 3 marked with the "border leaves to the right" flag (the host's 0 / 1 / 2 / 2 | -128), sixteen to a word
struct Cell2Px {
    unsigned* c;
    __device__ __forceinline__ int get(int i) const { return (int)((c[i >> 4] >> (2 * (i & 15))) & 3u); }
    __device__ __forceinline__ bool nz(int i) const { return get(i) != 0; }
    __device__ __forceinline__ bool one(int i) const { return get(i) == 1; }
    __device__ __forceinline__ void set(int i, bool end) { const unsigned sh = 2u * (unsigned)(i & 15); c[i >> 4] = (c[i >> 4] & ~(3u << sh)) | ((end ? 3u : 2u) << sh); }
};
// takes a border's points: the chain words, the bounding box and the area sum (prev x cur over consecutive points; the closing term is added by the caller)
struct ChainEmit {
    unsigned* out; int room, n, fx, fy, lx, ly, x0, y0, x1, y1; long long sum;
    __device__ __forceinline__ bool operator()(int x, int y) {
        if (n >= room) return false;
        out[n] = (unsigned)x | ((unsigned)y << 16);
        if (n == 0) { fx = x; fy = y; x0 = x1 = x; y0 = y1 = y; }
        else { sum += (long long)lx * y - (long long)ly * x; x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y); }
        lx = x; ly = y; n++;
        return true;
    }
};

__global__ void __launch_bounds__(64) k_piece_contours(const unsigned long long* __restrict__ planes, int W, int H, int wpr, PieceContourHdr* __restrict__ hdr_all,
                                                       unsigned* __restrict__ chain_all, PiecePlaneCount* __restrict__ count_all, int cap_contours, int cap_points,
                                                       unsigned* __restrict__ scratch, int use_lds, const int* __restrict__ gate, int gate_min) {
    extern __shared__ unsigned sm_cells[];
    const int lane = threadIdx.x, plane = blockIdx.x;
    if (gate && gate[plane] <= gate_min) { if (lane == 0) count_all[plane] = PiecePlaneCount{0, 0, PIECE_ST_OK, 0}; return; }
    const int w = W + 2, h = H + 2, ncell = w * h, nwords = (ncell + 15) >> 4;
    const unsigned long long* src = planes + (size_t)plane * H * wpr;
    unsigned* cells = use_lds ? sm_cells : scratch + (size_t)plane * nwords;
    PieceContourHdr* hdr = hdr_all + (size_t)plane * cap_contours; unsigned* chain = chain_all + (size_t)plane * cap_points;
    // the plane inside a frame of background, as cells
    for (int wi = lane; wi < nwords; wi += 64) {
        int c = wi << 4, y = c / w, x = c - y * w; unsigned v = 0u;
        for (int j = 0; j < 16; j++) {
            if (y >= 1 && y <= H && x >= 1 && x <= W) v |= (unsigned)((src[(size_t)(y - 1) * wpr + ((x - 1) >> 6)] >> ((x - 1) & 63)) & 1ull) << (2 * j);
            if (++x == w) { x = 0; y++; }
        }
        cells[wi] = v;
    }
    __threadfence_block(); __syncthreads();
    Cell2Px px{cells};
    const int end = (h - 1) * w;                        // rows 1 .. h - 2
    int pos = w + 1, prev = 0, lnbd_x = 0, row = 1, ncont = 0, npts = 0, status = PIECE_ST_OK;
    // every pass handles one change of value along the scan; a plane has fewer than ncell of them
    for (int pass = 0; pass < ncell; pass++) {
        int found = -1;
        const unsigned pat = (unsigned)prev * 0x55555555u;
        for (int base = pos >> 4; base < nwords; base += 64) {
            const int wi = base + lane;
            unsigned diff = wi < nwords ? cells[wi] ^ pat : 0u;
            diff = (diff | (diff >> 1)) & 0x55555555u;
            if (wi == (pos >> 4)) diff &= ~0u << (2 * (pos & 15));
            const unsigned long long b = __ballot(diff != 0u);
            if (b) {
                const int l = __ffsll((long long)b) - 1;
                const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)diff, l);
                found = ((base + l) << 4) + ((__ffs((int)d) - 1) >> 1);
                break;
            }
        }
        if (found < 0 || found >= end) break;
        const int y = found / w, x = found - y * w;
        if (y != row) { row = y; lnbd_x = 0; }          // (a row ends on its background column: the scan enters the next one with prev = 0)
        int p = px.get(found);
        bool start = prev == 0 && p == 1;
        if (!start && p == 0 && prev >= 1 && prev != 3 && (prev & 2)) lnbd_x = x - 1;      // a hole border would start here: not followed, but the scan remembers the mark it passed
        if (start) { const int q = px.get(y * w + lnbd_x); if (q == 1 || q == 2) start = false; }      // inside a border already followed (or a hole of it)
        if (start) {
            if (ncont >= cap_contours) { status = PIECE_ST_CONTOURS; break; }
            lnbd_x = x;
            int n = 0;
            if (lane == 0) {
                ChainEmit emit{chain + npts, cap_points - npts, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0ll};
                n = trace_border(px, w, found, x - 1, y - 1, false, emit, cap_points - npts);
                if (n > 0) {
                    long long s2 = emit.sum + ((long long)emit.lx * emit.fy - (long long)emit.ly * emit.fx); if (s2 < 0) s2 = -s2;
                    hdr[ncont] = PieceContourHdr{x - 1, y - 1, n, npts, emit.x0, emit.y0, emit.x1, emit.y1, (unsigned)(s2 & 0xffffffffll), (int)(s2 >> 32)};
                }
            }
            __threadfence_block(); __syncthreads();
            n = __builtin_amdgcn_readfirstlane(n);
            if (n < 0) { status = PIECE_ST_POINTS; break; }
            ncont++; npts += n;
            p = px.get(found);
        }
        prev = p;
        if (prev & 2) lnbd_x = x;
        pos = found + 1;
    }
    if (lane == 0) count_all[plane] = PiecePlaneCount{ncont, npts, status, 0};
}

int launch_piece_contours(hipStream_t s, const unsigned long long* planes, int nplanes, int W, int H, PieceContourHdr* hdr, unsigned* chain, PiecePlaneCount* count,
                          int cap_contours, int cap_points, unsigned* scratch, const int* gate, int gate_min) {
    if (!planes || !hdr || !chain || !count || nplanes < 1 || nplanes > 65535 || W < 1 || H < 1 || W > 8192 || H > 8192 || cap_contours < 1 || cap_points < 1) {
        sind_set_error("launch_piece_contours: %d planes of %d x %d, capacities %d / %d", nplanes, W, H, cap_contours, cap_points); return SIND_E_ARG; }
    const size_t bytes = piece_cell_words(W, H) * 4; const bool lds = bytes <= PIECE_LDS_BYTES;
    if (!lds && !scratch) { sind_set_error("launch_piece_contours: %d x %d needs the scratch plane", W, H); return SIND_E_ARG; }
    static SindPerDeviceInit attr_init;
    HIP_TRY(attr_init.run([] { return hipFuncSetAttribute((const void*)k_piece_contours, hipFuncAttributeMaxDynamicSharedMemorySize, PIECE_LDS_BYTES); }));
    hipLaunchKernelGGL(k_piece_contours, dim3(nplanes), dim3(64), lds ? bytes : 0, s, planes, W, H, (W + 63) / 64, hdr, chain, count, cap_contours, cap_points, scratch, lds ? 1 : 0, gate, gate_min);
    return SIND_OK;
}

// ================================================================================================================ the whole stage (PieceStage, pieces_dev.hpp)
typedef unsigned long long u64;

// elliptical dilation of one word of a bit plane given as a function (row, word) -> bits: dst(x, y) = OR over the element of src(x + j - ax, y + i - ay), positions
// outside the image ignored (the conventions of BitImg::dilated and k_dilate_planes)
template <class Src>
__device__ __forceinline__ u64 morph_dilate_word(Src src, int y, int k, int wpr, int H, const MorphElem& e, u64 tail_mask) {
    u64 acc = 0ull;
    for (int i = 0; i < e.n; i++) {
        const int ys = y + i - e.ay;
        if (ys < 0 || ys >= H || e.j2[i] <= e.j1[i]) continue;
        const u64 cur = src(ys, k), prev = k > 0 ? src(ys, k - 1) : 0ull, next = k + 1 < wpr ? src(ys, k + 1) : 0ull;
        for (int j = e.j1[i]; j < e.j2[i]; j++) {
            const int t = j - e.ax;
            if (t == 0) acc |= cur;
            else if (t > 0) acc |= (cur >> t) | (next << (64 - t));
            else acc |= (cur << (-t)) | (prev >> (64 + t));
        }
    }
    if (k == wpr - 1) acc &= tail_mask;
    return acc;
}

// blockIdx.y = 0: occDil = dilate(occ1, e10); 1 + i: tmp_i = erode_e4(label_i & ~occ1) = ~dilate(~X) inside the image.  blockIdx.z = frame
__global__ void __launch_bounds__(256) k_piece_prepare_a(const u64* __restrict__ in_planes, const u64* __restrict__ occ1, u64* __restrict__ occ_dil, u64* __restrict__ tmp,
                                                         const int* __restrict__ nplanes, int wpr, int H, MorphElem e10, MorphElem e4, u64 tm) {
    const size_t pw = (size_t)wpr * H; const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= pw) return;
    const int y = (int)(idx / wpr), k = (int)(idx - (size_t)y * wpr), b = blockIdx.z;
    const u64* o1 = occ1 + (size_t)b * pw;
    if (blockIdx.y == 0) { occ_dil[(size_t)b * pw + idx] = morph_dilate_word([&](int ys, int kk) { return o1[(size_t)ys * wpr + kk]; }, y, k, wpr, H, e10, tm); return; }
    const int i = blockIdx.y - 1;
    if (i >= nplanes[b]) return;
    const u64* lab = in_planes + ((size_t)b * PIECE_KMAX + i) * pw;
    auto inv = [&](int ys, int kk) { u64 v = ~(lab[(size_t)ys * wpr + kk] & ~o1[(size_t)ys * wpr + kk]); if (kk == wpr - 1) v &= tm; return v; };
    u64 r = ~morph_dilate_word(inv, y, k, wpr, H, e4, tm); if (k == wpr - 1) r &= tm;
    tmp[((size_t)b * PIECE_KMAX + i) * pw + idx] = r;
}
// each_i = dilate_e4(tmp_i): the opening's second half; planes the frame does not have come out empty
__global__ void __launch_bounds__(256) k_piece_prepare_b(const u64* __restrict__ tmp, u64* __restrict__ each, const int* __restrict__ nplanes, int wpr, int H, MorphElem e4, u64 tm) {
    const size_t pw = (size_t)wpr * H; const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= pw) return;
    const int y = (int)(idx / wpr), k = (int)(idx - (size_t)y * wpr), b = blockIdx.z, i = blockIdx.y;
    const size_t base = ((size_t)b * PIECE_KMAX + i) * pw;
    const u64* t = tmp + base;
    each[base + idx] = i < nplanes[b] ? morph_dilate_word([&](int ys, int kk) { return t[(size_t)ys * wpr + kk]; }, y, k, wpr, H, e4, tm) : 0ull;
}
// the pieces of a frame in discovery order: the contours of its planes, in order, that are long and large enough (size > 50, contourArea > 80 = |sum2| > 160).
// One wave per frame; a ballot numbers the 64 contours it looks at.
__global__ void __launch_bounds__(64) k_piece_index(const PieceContourHdr* __restrict__ hdr, const PiecePlaneCount* __restrict__ cnt, const int* __restrict__ nplanes, int cap_contours,
                                                    PieceRecDev* __restrict__ recs, PieceFrameHdr* __restrict__ frames, int* __restrict__ area, int* __restrict__ band) {
    const int b = blockIdx.x, lane = threadIdx.x; int C = 0, status = 0;
    const int np = min(max(nplanes[b], 0), PIECE_KMAX);
    for (int i = 0; i < np; i++) {
        const PiecePlaneCount c = cnt[b * PIECE_KMAX + i];
        if (c.status) status = c.status;
        const int nc = min(max(c.contours, 0), cap_contours);
        for (int base = 0; base < nc; base += 64) {
            const int ci = base + lane; bool keep = false; PieceContourHdr h = {};
            if (ci < nc) { h = hdr[(size_t)(b * PIECE_KMAX + i) * cap_contours + ci]; const long long s2 = ((long long)h.sum2_hi << 32) | (long long)h.sum2_lo; keep = h.len > 50 && s2 > 160; }
            const u64 m = __ballot(keep);
            const int slot = C + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && slot < PIECE_SLOTS) recs[(size_t)b * PIECE_SLOTS + slot] = PieceRecDev{i, ci, h.sx, h.sy, h.len, h.x0, h.y0, h.x1, h.y1, h.sum2_lo, h.sum2_hi, 0, 0, 0, 0.f, 0};
            C += __popcll(m);
        }
    }
    for (int s = lane; s < PIECE_SLOTS; s += 64) { area[b * PIECE_SLOTS + s] = 0; band[b * PIECE_SLOTS + s] = 0; }
    if (lane == 0) frames[b] = PieceFrameHdr{C, status, 0, 0};
}
// zero up to four plane sets of the frame's pieces.  grid (words, PIECE_SLOTS, frames)
__global__ void __launch_bounds__(256) k_piece_clear(const PieceFrameHdr* __restrict__ frames, u64* __restrict__ a, u64* __restrict__ b2, u64* __restrict__ c, u64* __restrict__ d, size_t pw) {
    const int slot = blockIdx.y, b = blockIdx.z;
    if (slot >= min(frames[b].pieces, PIECE_SLOTS)) return;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= pw) return;
    const size_t o = ((size_t)b * PIECE_SLOTS + slot) * pw + idx;
    if (a) a[o] = 0ull; if (b2) b2[o] = 0ull; if (c) c[o] = 0ull; if (d) d[o] = 0ull;
}
__device__ __forceinline__ void plane_or(u64* p, int wpr, int W, int H, int x, int y) { if (x >= 0 && y >= 0 && x < W && y < H) atomicOr(p + (size_t)y * wpr + (x >> 6), 1ull << (x & 63)); }
// one closed chain into a contour plane and a crossing plane (draw_filled's edge table as bits: an edge that changes row toggles the bit of its upper end; two equal
// crossings cancel, and their pixel is a contour pixel anyway)
__device__ __forceinline__ void chain_draw(const unsigned* __restrict__ ch, int L, u64* cont, u64* cross, u64* bandp, int wpr, int W, int H) {
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        const unsigned p = ch[i], q = ch[i + 1 < L ? i + 1 : 0];
        const int px = (int)(p & 0xffffu), py = (int)(p >> 16), qx = (int)(q & 0xffffu), qy = (int)(q >> 16);
        plane_or(cont, wpr, W, H, px, py);
        if (py != qy) { const int tx = py < qy ? px : qx, ty = py < qy ? py : qy; if (tx >= 0 && ty >= 0 && tx < W && ty < H) atomicXor(cross + (size_t)ty * wpr + (tx >> 6), 1ull << (tx & 63)); }
        if (bandp) { plane_or(bandp, wpr, W, H, px, py); plane_or(bandp, wpr, W, H, px - 1, py); plane_or(bandp, wpr, W, H, px + 1, py); plane_or(bandp, wpr, W, H, px, py - 1); plane_or(bandp, wpr, W, H, px, py + 1); }
    }
}
// every piece's contour: contour bits into pa, crossings into pb, the thickness-2 band (draw_thick2's five-pixel cross) into pc.  grid (PIECE_SLOTS, frames)
__global__ void __launch_bounds__(256) k_piece_draw(const PieceFrameHdr* __restrict__ frames, const PieceRecDev* __restrict__ recs, const PieceContourHdr* __restrict__ hdr,
                                                    const unsigned* __restrict__ chain, int cap_contours, int cap_points, u64* __restrict__ pa, u64* __restrict__ pb, u64* __restrict__ pc,
                                                    int wpr, int W, int H) {
    const int slot = blockIdx.x, b = blockIdx.y;
    if (slot >= min(frames[b].pieces, PIECE_SLOTS)) return;
    const PieceRecDev r = recs[(size_t)b * PIECE_SLOTS + slot];
    const size_t pl = (size_t)b * PIECE_KMAX + r.cluster, pw = (size_t)wpr * H, o = ((size_t)b * PIECE_SLOTS + slot) * pw;
    const PieceContourHdr h = hdr[pl * cap_contours + r.contour];
    if (h.off < 0 || h.len < 1 || h.off + h.len > cap_points) return;
    chain_draw(chain + pl * cap_points + h.off, h.len, pa + o, pb + o, pc + o, wpr, W, H);
}
// per (piece, row): cont |= inclusive prefix parity of the crossings (a pair of crossings fills from the first to the pixel before the second, which is a contour pixel).
// One thread per row.  grid (rows / 256, PIECE_SLOTS, frames)
__global__ void __launch_bounds__(256) k_piece_fill(const PieceFrameHdr* __restrict__ frames, u64* __restrict__ cont, const u64* __restrict__ cross, int wpr, int H) {
    const int slot = blockIdx.y, b = blockIdx.z;
    if (slot >= min(frames[b].pieces, PIECE_SLOTS)) return;
    const int y = blockIdx.x * 256 + threadIdx.x;
    if (y >= H) return;
    const size_t o = (((size_t)b * PIECE_SLOTS + slot) * H + y) * wpr;
    unsigned carry = 0u;
    for (int k = 0; k < wpr; k++) {
        const u64 x = cross[o + k]; u64 pre = x;
        pre ^= pre << 1; pre ^= pre << 2; pre ^= pre << 4; pre ^= pre << 8; pre ^= pre << 16; pre ^= pre << 32;
        if (carry) pre = ~pre;
        carry ^= (unsigned)__popcll(x) & 1u;
        cont[o + k] |= pre;
    }
}
// piece = dilate_e9(fill) & original cluster plane, counted; t1 = band & ~occDil & labelForSegEdge, counted.  pa: fill (read), pb: the piece (written), pc: band -> t1
__global__ void __launch_bounds__(256) k_piece_grow(const PieceFrameHdr* __restrict__ frames, const PieceRecDev* __restrict__ recs, const u64* __restrict__ pa, u64* __restrict__ pb, u64* __restrict__ pc,
                                                    const u64* __restrict__ in_planes, const u64* __restrict__ occ_dil, const u64* __restrict__ label_edge,
                                                    int* __restrict__ area, int* __restrict__ band, int wpr, int H, MorphElem e9, u64 tm) {
    const int slot = blockIdx.y, b = blockIdx.z;
    if (slot >= min(frames[b].pieces, PIECE_SLOTS)) return;
    const size_t pw = (size_t)wpr * H; const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= pw) return;
    const int y = (int)(idx / wpr), k = (int)(idx - (size_t)y * wpr);
    const size_t o = ((size_t)b * PIECE_SLOTS + slot) * pw;
    const u64* fill = pa + o;
    const int cl = recs[(size_t)b * PIECE_SLOTS + slot].cluster;
    const u64 img = morph_dilate_word([&](int ys, int kk) { return fill[(size_t)ys * wpr + kk]; }, y, k, wpr, H, e9, tm) & in_planes[((size_t)b * PIECE_KMAX + cl) * pw + idx];
    pb[o + idx] = img;
    if (img) atomicAdd(area + b * PIECE_SLOTS + slot, __popcll(img));
    const u64 t1 = pc[o + idx] & ~occ_dil[(size_t)b * pw + idx] & label_edge[(size_t)b * pw + idx];
    pc[o + idx] = t1;
    if (t1) atomicAdd(band + b * PIECE_SLOTS + slot, __popcll(t1));
}
// second level: every contour of a piece's t1 plane with 30 points or more goes into ONE contour plane (pa) and ONE crossing plane (pd): even-odd over all of them.
// Also completes the record (area, band count, hasLianjie) and passes a capacity status of the second level on to the frame
__global__ void __launch_bounds__(256) k_piece_draw2(PieceFrameHdr* __restrict__ frames, PieceRecDev* __restrict__ recs, const PieceContourHdr* __restrict__ hdr2, const unsigned* __restrict__ chain2,
                                                     const PiecePlaneCount* __restrict__ cnt2, int cap_contours2, int cap_points2, u64* __restrict__ pa, u64* __restrict__ pd,
                                                     const int* __restrict__ area, const int* __restrict__ band, int wpr, int W, int H) {
    const int slot = blockIdx.x, b = blockIdx.y;
    if (slot >= min(frames[b].pieces, PIECE_SLOTS)) return;
    const size_t ps = (size_t)b * PIECE_SLOTS + slot, o = ps * (size_t)wpr * H;
    const PiecePlaneCount c = cnt2[ps];
    const int nc = min(max(c.contours, 0), cap_contours2);
    bool kept = false;
    for (int q = 0; q < nc; q++) {
        const PieceContourHdr h = hdr2[ps * cap_contours2 + q];
        if (h.len < 30 || h.off < 0 || h.off + h.len > cap_points2) continue;
        kept = true;
        chain_draw(chain2 + ps * cap_points2 + h.off, h.len, pa + o, pd + o, nullptr, wpr, W, H);
    }
    if (threadIdx.x == 0) {
        recs[ps].area = area[ps]; recs[ps].band = band[ps]; recs[ps].has_conn = kept ? 1 : 0;
        if (c.status) atomicOr(&frames[b].status, 4);
    }
}
// myCluster::calCenterPoint's z (DD:256-293): the FP32 sum of (float)d * invDepthScale * 1.5f over the piece's pixels in row-major order, one add after the other, product
// and add separate; a raw depth of 0 or >= z_invalid adds 0.  One wave per piece: 64 plane words are fetched at once, the lanes of a word's 64 pixels form their terms,
// and the running sum takes them in bit order.
// Frame b's depth plane: depth_tab[b] where a table is given (a chunk's frames come from arbitrary streams), else depth + b * depth_stride.
__global__ void __launch_bounds__(64) k_piece_centre(const PieceFrameHdr* __restrict__ frames, PieceRecDev* __restrict__ recs, const u64* __restrict__ pb, const uint16_t* __restrict__ depth,
                                                     size_t depth_stride, const uint16_t* const* __restrict__ depth_tab, int z_invalid, float inv_scale, int wpr, int W, int H) {
    const int slot = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (slot >= min(frames[b].pieces, PIECE_SLOTS)) return;
    const size_t ps = (size_t)b * PIECE_SLOTS + slot; const int pw = wpr * H;
    const u64* img = pb + ps * (size_t)pw; const uint16_t* dp = depth_tab ? depth_tab[b] : depth + (size_t)b * depth_stride;
    float f3 = 0.f;
    for (int base = 0; base < pw; base += 64) {
        const int wi = base + lane;
        const u64 mine = wi < pw ? img[wi] : 0ull;
        u64 nz = __ballot(mine != 0ull);
        while (nz) {
            const int l = __ffsll((long long)nz) - 1; nz &= nz - 1;
            const u64 m = ((u64)(unsigned)__builtin_amdgcn_readlane((int)(mine >> 32), l) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane((int)mine, l);
            const int widx = base + l, y = widx / wpr, x = ((widx - y * wpr) << 6) + lane;
            float v = 0.f;
            if (((m >> lane) & 1ull) && x < W) { const int d = dp[(size_t)y * W + x]; if (!(d >= z_invalid || d == 0)) { const float depth2 = (float)d * inv_scale; v = depth2 * 1.5f; } }
            u64 bits = m;
            while (bits) { const int q = __ffsll((long long)bits) - 1; bits &= bits - 1; f3 += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), q)); }
        }
    }
    if (lane == 0) recs[ps].cz = f3 / (float)recs[ps].area;
}

// ---- k_piece_commit: the ranked pieces into the RAG stage's plane layout, and pieceOf
__global__ void __launch_bounds__(256) k_piece_commit(const u64* __restrict__ pb, const u64* __restrict__ pa, const int* __restrict__ order, const int* __restrict__ has_conn,
                                                      u64* __restrict__ out, int C, size_t pw) {
    const int r = blockIdx.y; const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= C || idx >= pw) return;
    const int slot = order[r];
    if (slot < 0 || slot >= PIECE_SLOTS) return;
    out[(size_t)r * pw + idx] = pb[(size_t)slot * pw + idx];
    out[((size_t)2 * C + r) * pw + idx] = has_conn[r] ? pa[(size_t)slot * pw + idx] : 0ull;
}
// one thread per pixel; the 64 lanes of a wave read the same plane word (W % 64 == 0 in the tail; any W works)
__global__ void __launch_bounds__(256) k_piece_paint(const u64* __restrict__ pb, const int* __restrict__ order, uint8_t* __restrict__ piece_of, int C, int W, int H, int wpr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= W * H) return;
    const int y = i / W, x = i - y * W; const size_t widx = (size_t)y * wpr + (x >> 6), pw = (size_t)wpr * H;
    int owner = C + 1;
    for (int r = C - 1; r >= 0; r--) {
        const int slot = order[r];
        if (slot < 0 || slot >= PIECE_SLOTS) continue;
        if ((pb[(size_t)slot * pw + widx] >> (x & 63)) & 1ull) { owner = r; break; }
    }
    piece_of[i] = (uint8_t)owner;
}
int launch_piece_commit(hipStream_t s, const PieceStage& st, int b, int C, const int* order_dev, const int* has_conn_dev, unsigned long long* planes_out, uint8_t* piece_of_out) {
    if (b < 0 || b >= st.cap || C < 1 || C > 254 || !order_dev || !has_conn_dev || !planes_out || !piece_of_out) { sind_set_error("launch_piece_commit: frame %d, %d pieces", b, C); return SIND_E_ARG; }
    const u64* pb = st.pb.p + (size_t)b * PIECE_SLOTS * st.pw; const u64* pa = st.pa.p + (size_t)b * PIECE_SLOTS * st.pw;
    hipLaunchKernelGGL(k_piece_commit, dim3((unsigned)((st.pw + 255) / 256), C), dim3(256), 0, s, pb, pa, order_dev, has_conn_dev, planes_out, C, st.pw);
    hipLaunchKernelGGL(k_piece_paint, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, s, pb, order_dev, piece_of_out, C, st.W, st.H, st.wpr);
    return SIND_OK;
}

// ---- the same for the frames of a chunk, into the batched RAG stage's slab (PieceCommitRec, pieces_dev.hpp).  grid (words, the chunk's largest C, frames)
__global__ void __launch_bounds__(256) k_piece_commit_frames(const PieceCommitRec* __restrict__ recs, const int* __restrict__ table, const u64* __restrict__ pb, const u64* __restrict__ pa,
                                                             u64* __restrict__ slab, size_t pw) {
    const PieceCommitRec R = recs[blockIdx.z];
    const int r = blockIdx.y; const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R.C || idx >= pw) return;
    const int slot = table[R.tab_off + r];
    if (slot < 0 || slot >= PIECE_SLOTS) return;
    const size_t src = ((size_t)R.b * PIECE_SLOTS + slot) * pw + idx;
    u64* out = slab + R.plane_off;
    out[(size_t)r * pw + idx] = pb[src];
    out[((size_t)R.C + r) * pw + idx] = table[R.tab_off + PIECE_SLOTS + r] ? pa[src] : 0ull;
}
// pieceOf of a chunk's frames.  k_piece_paint walks the ranks from the top with one dependent load per rank and pixel; the 64 pixels of a plane word read the SAME word
// of every rank, so here a wave owns one word position: its lanes load that word from 64 ranks at once (lane l: rank top - l), a ballot names the ranks whose word is not
// empty -- a few of the C, pieces overlap little -- and only those are looked at, highest rank first; a pixel keeps the first rank that has its bit.  Same result: the
// owner is the highest rank whose plane has the pixel.  Four waves per workgroup; grid (words / 4, frames)
__global__ void __launch_bounds__(256) k_piece_paint_frames(const PieceCommitRec* __restrict__ recs, const int* __restrict__ table, const u64* __restrict__ pb,
                                                            uint8_t* __restrict__ piece_of, int W, int H, int wpr) {
    const PieceCommitRec R = recs[blockIdx.y];
    const int lane = threadIdx.x & 63; const size_t pw = (size_t)wpr * H; const size_t widx = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (widx >= pw) return;                         // (the whole wave)
    const int y = (int)(widx / wpr), x = ((int)(widx - (size_t)y * wpr) << 6) + lane;
    const u64* planes = pb + (size_t)R.b * PIECE_SLOTS * pw + widx;
    int owner = -1;
    for (int top = R.C - 1; top >= 0; top -= 64) {
        const int r = top - lane; u64 mine = 0ull;
        if (r >= 0) { const int slot = table[R.tab_off + r]; if (slot >= 0 && slot < PIECE_SLOTS) mine = planes[(size_t)slot * pw]; }
        u64 nz = __ballot(mine != 0ull);
        while (nz) {
            const int l = __ffsll((long long)nz) - 1; nz &= nz - 1;
            const u64 m = ((u64)(unsigned)__builtin_amdgcn_readlane((int)(mine >> 32), l) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane((int)mine, l);
            if (owner < 0 && ((m >> lane) & 1ull)) owner = top - l;
        }
        if (__ballot(owner < 0) == 0ull) break;
    }
    if (x < W) piece_of[R.piece_of_off + (size_t)y * W + x] = (uint8_t)(owner < 0 ? R.C + 1 : owner);
}
int launch_piece_commit_frames(hipStream_t s, const PieceStage& st, const PieceCommitRec* recs_dev, const PieceCommitRec* host, int n, const int* table_dev, size_t table_ints,
                               unsigned long long* slab, size_t slab_words, uint8_t* piece_of, size_t piece_of_bytes) {
    if (n < 1 || n > st.cap || !recs_dev || !host || !table_dev || !slab || !piece_of) { sind_set_error("launch_piece_commit_frames: %d frames (capacity %d) or a null pointer", n, st.cap); return SIND_E_ARG; }
    int maxC = 0;
    for (int i = 0; i < n; i++) {
        const PieceCommitRec& R = host[i];
        if (R.b < 0 || R.b >= st.cap || R.C < 1 || R.C > 254 || R.tab_off < 0 || (size_t)R.tab_off + 2 * PIECE_SLOTS > table_ints || R.plane_off + (size_t)2 * R.C * st.pw > slab_words ||
            R.piece_of_off + st.N > piece_of_bytes) { sind_set_error("launch_piece_commit_frames: record %d (frame %d, %d pieces) leaves the stage, its table, the slab or pieceOf", i, R.b, R.C); return SIND_E_ARG; }
        maxC = std::max(maxC, R.C);
    }
    hipLaunchKernelGGL(k_piece_commit_frames, dim3((unsigned)((st.pw + 255) / 256), maxC, n), dim3(256), 0, s, recs_dev, table_dev, st.pb.p, st.pa.p, slab, st.pw);
    hipLaunchKernelGGL(k_piece_paint_frames, dim3((unsigned)((st.pw + 3) / 4), n), dim3(256), 0, s, recs_dev, table_dev, st.pb.p, piece_of, st.W, st.H, st.wpr);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int PieceStage::enqueue(hipStream_t s, int n, const uint16_t* depth_dev, size_t depth_stride, int z_invalid_from, float inv_depth_scale, const uint16_t* const* depth_tab) {
    if (n < 1 || n > cap) { sind_set_error("PieceStage::enqueue: %d frames, capacity %d", n, cap); return SIND_E_ARG; }
    const u64 tm = (W & 63) ? ((1ull << (W & 63)) - 1) : ~0ull;
    const unsigned gw = (unsigned)((pw + 255) / 256);
    const MorphElem e4 = make_ellipse(4), e9 = make_ellipse(9), e10 = make_ellipse(10);
    if (!depth_dev) { depth_dev = depth.p; depth_stride = N; }
    hipLaunchKernelGGL(k_piece_prepare_a, dim3(gw, PIECE_KMAX + 1, n), dim3(256), 0, s, in_planes.p, occ1.p, occ_dil.p, tmp.p, nplanes_d.p, wpr, H, e10, e4, tm);
    hipLaunchKernelGGL(k_piece_prepare_b, dim3(gw, PIECE_KMAX, n), dim3(256), 0, s, tmp.p, each.p, nplanes_d.p, wpr, H, e4, tm);
    SIND_TRY(launch_piece_contours(s, each.p, n * PIECE_KMAX, W, H, l1.hdr.p, l1.chain.p, l1.count.p, l1.cap_contours, l1.cap_points, l1.scratch.p));
    hipLaunchKernelGGL(k_piece_index, dim3(n), dim3(64), 0, s, l1.hdr.p, l1.count.p, nplanes_d.p, l1.cap_contours, recs.p, frames.p, area.p, band.p);
    hipLaunchKernelGGL(k_piece_clear, dim3(gw, PIECE_SLOTS, n), dim3(256), 0, s, frames.p, pa.p, pb.p, pc.p, pd.p, pw);
    hipLaunchKernelGGL(k_piece_draw, dim3(PIECE_SLOTS, n), dim3(256), 0, s, frames.p, recs.p, l1.hdr.p, l1.chain.p, l1.cap_contours, l1.cap_points, pa.p, pb.p, pc.p, wpr, W, H);
    hipLaunchKernelGGL(k_piece_fill, dim3((H + 255) / 256, PIECE_SLOTS, n), dim3(256), 0, s, frames.p, pa.p, pb.p, wpr, H);
    hipLaunchKernelGGL(k_piece_grow, dim3(gw, PIECE_SLOTS, n), dim3(256), 0, s, frames.p, recs.p, pa.p, pb.p, pc.p, in_planes.p, occ_dil.p, label_edge.p, area.p, band.p, wpr, H, e9, tm);
    SIND_TRY(launch_piece_contours(s, pc.p, n * PIECE_SLOTS, W, H, l2.hdr.p, l2.chain.p, l2.count.p, l2.cap_contours, l2.cap_points, l2.scratch.p, band.p, 20));
    hipLaunchKernelGGL(k_piece_clear, dim3(gw, PIECE_SLOTS, n), dim3(256), 0, s, frames.p, pa.p, (u64*)nullptr, (u64*)nullptr, (u64*)nullptr, pw);
    hipLaunchKernelGGL(k_piece_draw2, dim3(PIECE_SLOTS, n), dim3(256), 0, s, frames.p, recs.p, l2.hdr.p, l2.chain.p, l2.count.p, l2.cap_contours, l2.cap_points, pa.p, pd.p, area.p, band.p, wpr, W, H);
    hipLaunchKernelGGL(k_piece_fill, dim3((H + 255) / 256, PIECE_SLOTS, n), dim3(256), 0, s, frames.p, pa.p, pd.p, wpr, H);
    hipLaunchKernelGGL(k_piece_centre, dim3(PIECE_SLOTS, n), dim3(64), 0, s, frames.p, recs.p, pb.p, depth_dev, depth_stride, depth_tab, z_invalid_from, inv_depth_scale, wpr, W, H);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
