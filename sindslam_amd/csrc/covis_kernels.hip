// The covisibility table on the GPU (include/sind_hip.h "sind_covis_*"; reference src/KeyFrame.cc:289-320, src/Tracking.cc:1268-1288, src/LocalMapping.cc:645-691).
// The per-element steps are host/covis.hpp, the source the host twin compiles too; this file is how they are spread over lanes.
//   k_covis_apply   one lane per op.  No two ops of a call name one cell (checked on the host), so the cell is exchanged with plain loads and stores; the aggregates of
//                   a point are shared by its ops and move with integer atomics: exact in any order.
//   k_covis_tag     one lane per list entry: atomicOr of the entry's bit into the point's tag word.
//   k_covis_count   one wave per (key-frame row, 64 bits).  The lanes read 64 cells of the row at a time (coalesced), gather the tag word of each cell's point, and
//                   every bit is summed with one ballot and popcount; lane b keeps the sum of bit b.  A group of 64 cells without any tag costs one ballot.  Nothing
//                   is atomic and nothing depends on how many observations a point has: a pass costs rows * cap_feat cell reads.
//   k_covis_untag   the same entries, atomicAnd with the complement: the tags are zero again without a pass over cap_points.
//   k_covis_cull    one lane per entry of all items.  The lane finds its item by bisection over the item starts, evaluates covis_cull_entry, and the two counts of
//                   an item are summed per wave with ballots (an item's entries are consecutive, a wave meets a few items at most) and added with one atomic per
//                   (wave, item).
#include "covis_dev.hpp"

namespace sind {

#define CV_NT 256

namespace {
struct AtomicAdd { __device__ void operator()(int* p, int v) const { atomicAdd(p, v); } };
}

__global__ __launch_bounds__(CV_NT) void k_covis_apply(CovisTable t, const ::sind_covis_op* ops, int n) {
    const int i = blockIdx.x * CV_NT + threadIdx.x;
    if (i < n) covis_exchange(t, ops[i], AtomicAdd());
}

__global__ __launch_bounds__(CV_NT) void k_covis_tag(unsigned long long* tag, const int* entPoint, const int* entBit, int n, int capPoints) {
    const int i = blockIdx.x * CV_NT + threadIdx.x;
    if (i < n) atomicOr(tag + (size_t)covis_tag_word(entBit[i]) * capPoints + entPoint[i], covis_tag_mask(entBit[i]));
}

__global__ __launch_bounds__(CV_NT) void k_covis_untag(unsigned long long* tag, const int* entPoint, const int* entBit, int n, int capPoints) {
    const int i = blockIdx.x * CV_NT + threadIdx.x;
    if (i < n) atomicAnd(tag + (size_t)covis_tag_word(entBit[i]) * capPoints + entPoint[i], ~covis_tag_mask(entBit[i]));
}

__global__ __launch_bounds__(CV_NT) void k_covis_count(CovisTable t, const unsigned long long* tag, int* perBit, int rows, int nBits) {
    const int lane = threadIdx.x & 63, kf = __builtin_amdgcn_readfirstlane(blockIdx.x * (CV_NT / 64) + (threadIdx.x >> 6)), word = blockIdx.y;
    if (kf >= rows) return;
    const int bits = min(64, nBits - word * 64);
    const int* row = t.cellPoint + (size_t)kf * t.capFeat; const unsigned long long* tw = tag + (size_t)word * t.capPoints;
    int sum = 0;                                                      // lane b: the sum of bit b
    for (int c0 = 0; c0 < t.capFeat; c0 += 64) {
        const int i = c0 + lane;
        const unsigned long long m = i < t.capFeat ? covis_cell_tags(row, i, tw) : 0ull;
        if (!__ballot(m != 0)) continue;
        for (int b = 0; b < bits; b++) {
            const int c = __popcll(__ballot((m >> b) & 1));
            if (lane == b) sum += c;
        }
    }
    if (lane < bits) perBit[(size_t)(word * 64 + lane) * rows + kf] = sum;
}

__global__ __launch_bounds__(CV_NT) void k_covis_cull(CovisTable t, const int* itemStart, const int* itemKf, int B, const int* entPoint, const uint8_t* entOctave,
                                                      const uint8_t* entClose, int n, int thObs, int* counts, uint8_t* redundant) {
    const int e = blockIdx.x * CV_NT + threadIdx.x, lane = threadIdx.x & 63;
    int item = -1, mps = 0, red = 0;
    if (e < n) {
        int lo = 0, hi = B;                                           // the last item that starts at or before e: itemStart[lo] <= e < itemStart[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (itemStart[mid] <= e) lo = mid; else hi = mid; }
        item = lo;
        const int p = entPoint[e];
        if (p >= 0 && entClose[e]) { mps = 1; red = covis_cull_entry(t, itemKf[item], e - itemStart[item], p, entOctave[e], thObs); }
        redundant[e] = (uint8_t)red;
    }
    for (unsigned long long todo = __ballot(item >= 0); todo;) {
        const int it = __builtin_amdgcn_readlane(item, __builtin_ctzll(todo));
        const unsigned long long mine = __ballot(item == it);
        const int cm = __popcll(__ballot(item == it && mps)), cr = __popcll(__ballot(item == it && red));
        if (lane == __builtin_ctzll(mine)) { if (cm) atomicAdd(&counts[2 * it], cm); if (cr) atomicAdd(&counts[2 * it + 1], cr); }
        todo &= ~mine;
    }
}

int launch_covis_apply(const CovisTable& t, const ::sind_covis_op* ops, int n, hipStream_t s) {
    if (!n) return SIND_OK;
    hipLaunchKernelGGL(k_covis_apply, dim3(divup(n, CV_NT)), dim3(CV_NT), 0, s, t, ops, n);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_covis_tag(unsigned long long* tag, const int* entPoint, const int* entBit, int n, int capPoints, bool set, hipStream_t s) {
    if (!n) return SIND_OK;
    if (set) hipLaunchKernelGGL(k_covis_tag, dim3(divup(n, CV_NT)), dim3(CV_NT), 0, s, tag, entPoint, entBit, n, capPoints);
    else hipLaunchKernelGGL(k_covis_untag, dim3(divup(n, CV_NT)), dim3(CV_NT), 0, s, tag, entPoint, entBit, n, capPoints);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_covis_count(const CovisTable& t, const unsigned long long* tag, int* perBit, int rows, int nBits, hipStream_t s) {
    if (!rows || !nBits) return SIND_OK;
    hipLaunchKernelGGL(k_covis_count, dim3(divup(rows, CV_NT / 64), divup(nBits, 64)), dim3(CV_NT), 0, s, t, tag, perBit, rows, nBits);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_covis_cull(const CovisTable& t, const int* itemStart, const int* itemKf, int B, const int* entPoint, const uint8_t* entOctave, const uint8_t* entClose, int n,
                      int thObs, int* counts, uint8_t* redundant, hipStream_t s) {
    if (!n) return SIND_OK;
    hipLaunchKernelGGL(k_covis_cull, dim3(divup(n, CV_NT)), dim3(CV_NT), 0, s, t, itemStart, itemKf, B, entPoint, entOctave, entClose, n, thObs, counts, redundant);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
