// The feature-vector half of Frame::ComputeBoW / KeyFrame::ComputeBoW on the GPU: TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)
// (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259) for every descriptor of B frames, with FORB::distance = Hamming distance.
// One thread per descriptor, its 32 bytes in registers; the tree (CSR children, 32 B per node) is read through the caches: the top levels are shared
// by every thread, and a descent touches levels * k nodes.  Integer work only, so the result is the reference's bit for bit.
//   descent   from the root, at every level the child of smallest distance, strict '<' in the children's order (the first child wins a tie), until a
//             childless node; word_id = that leaf's word
//   node_id   the node passed at level (levels - levelsup); 0 when that level is <= 0; the leaf itself when the path ends above that level (the
//             reference leaves nid uninitialised there); -1 when the word is stopped, !(weight > 0), which keeps the feature out of mFeatVec (:1157-1161)
// The BowVector half (transform(features, v, fv, levelsup) :1127-1194 with BowVector::addWeight, BowVector.cpp:34-46, and BowVector::normalize, :62-84; TF_IDF
// weighting and L1 norm, the ORB vocabulary's): k_voc_transform<true> also leaves the leaf every descriptor ended on, and k_bow_vector, one workgroup per
// frame, turns them into the std::map<WordId, WordValue> without leaving the device:
//   sort      (word, feature index) keys of the features whose leaf has weight > 0, bitonic in LDS as k_bow_group sorts (node, index) (match_bow.hip)
//   add       one lane per distinct word walks the word's entries in feature order: w, w + w, (w + w) + w, ... in FP64, each term the weight of that
//             feature's leaf (addWeight is called once per feature; the sum is not count * w)
//   compact   the words' ranks from a workgroup prefix sum; the values take the keys' place in LDS
//   norm      one lane adds fabs(value) over ascending word id, left to right (the map's iteration order)
//   divide    value / norm (IEEE FP64) if norm > 0
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

#define VT_NT 256

template <bool LEAF>
__global__ __launch_bounds__(VT_NT) void k_voc_transform(VocTree tr, const uint32_t* desc, const int* n, int cap, int nidLevel, int* nodeId, int* wordId, int* leafId) {
    const int b = blockIdx.y, i = blockIdx.x * VT_NT + threadIdx.x;
    if (i >= min(n[b], cap)) return;
    const size_t o = (size_t)b * cap + i;
    const uint4 d0 = *(const uint4*)(desc + 8 * o), d1 = *(const uint4*)(desc + 8 * o + 4);
    int node = 0, nid = nidLevel <= 0 ? 0 : -1;
    for (int level = 1; level <= tr.nNodes; level++) {             // a validated tree ends every path long before; the bound only makes that plain
        const int cb = tr.childStart[node], ce = tr.childStart[node + 1];
        if (cb == ce) break;
        int best = tr.child[cb], bestD = d_hamming(tr.desc + 8 * (size_t)best, d0, d1);
        for (int j = cb + 1; j < ce; j++) {
            const int c = tr.child[j], d = d_hamming(tr.desc + 8 * (size_t)c, d0, d1);
            if (d < bestD) { bestD = d; best = c; }
        }
        node = best;
        if (level == nidLevel) nid = node;
    }
    if (nid < 0) nid = node;
    nodeId[o] = tr.stopped[node] ? -1 : nid;
    wordId[o] = tr.wordId[node];
    if (LEAF) leafId[o] = node;
}

#define BV_NT 1024
#define BV_PER (BOW_MAX_KEYS / BV_NT)                              // sorted positions per thread when a frame fills the capacity

__global__ __launch_bounds__(BV_NT) void k_bow_vector(const double* weight, const int* n, int cap, int sortLen, const int* wordId, const int* leafId, int* bowWord, double* bowValue,
                                                      int* nWords) {
    extern __shared__ unsigned long long keys[];                   // word << 32 | feature index, sortLen of them; later the values, one double per distinct word
    __shared__ int words[BOW_MAX_KEYS], waveSum[BV_NT / 64], total;
    __shared__ double normSh;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, nb = min(min(n[b], cap), sortLen);
    const size_t o = (size_t)b * cap;
    for (int i = t; i < sortLen; i += BV_NT)
        keys[i] = (i < nb && weight[leafId[o + i]] > 0) ? ((unsigned long long)(uint32_t)wordId[o + i] << 32) | (uint32_t)i : ~0ull;      // stopped words are absent
    __syncthreads();
    for (int k = 2; k <= sortLen; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < sortLen; i += BV_NT) {
                const int p = i ^ j;
                if (p > i) { const unsigned long long x = keys[i], y = keys[p]; if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[p] = x; } }
            }
            __syncthreads();
        }
    // a thread owns `per` consecutive sorted positions; where one is the first entry of a word, the thread adds that word's weights in feature order
    const int per = max(1, sortLen / BV_NT), base = t * per;
    int w[BV_PER], heads = 0; double v[BV_PER];
#pragma unroll
    for (int k = 0; k < BV_PER; k++) {
        const int i = base + k; w[k] = 0; v[k] = 0.0;
        if (k >= per || i >= sortLen) continue;
        const unsigned long long key = keys[i];
        if (key == ~0ull || (i > 0 && (keys[i - 1] >> 32) == (key >> 32))) continue;
        double s = weight[leafId[o + (uint32_t)key]];
        for (int j = i + 1; j < sortLen && (keys[j] >> 32) == (key >> 32); j++) s = s + weight[leafId[o + (uint32_t)keys[j]]];
        w[k] = (int)(key >> 32); v[k] = s; heads |= 1 << k;
    }
    const int c = __popc(heads);
    int incl = c;
    for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(incl, d); if (lane >= d) incl += u; }
    if (lane == 63) waveSum[wave] = incl;
    __syncthreads();                                               // and nobody reads a key any more
    int r = incl - c;
    for (int q = 0; q < wave; q++) r += waveSum[q];
    if (t == BV_NT - 1) total = r + c;
    double* vals = (double*)keys;
#pragma unroll
    for (int k = 0; k < BV_PER; k++) if ((heads >> k) & 1) { words[r] = w[k]; vals[r] = v[k]; r++; }
    __syncthreads();
    const int nw = total;
    if (t == 0) {
        double norm = 0.0;
        for (int i = 0; i < nw; i++) norm = norm + fabs(vals[i]);
        normSh = norm; nWords[b] = nw;
    }
    __syncthreads();
    const double norm = normSh;
    for (int i = t; i < nw; i += BV_NT) { bowWord[o + i] = words[i]; bowValue[o + i] = norm > 0.0 ? vals[i] / norm : vals[i]; }
}

int launch_voc_transform(const VocTree& tree, const uint32_t* desc, const int* n, int cap, int maxN, int B, int nidLevel, int* nodeId, int* wordId, hipStream_t s) {
    hipLaunchKernelGGL(k_voc_transform<false>, dim3(divup(maxN, VT_NT), B), dim3(VT_NT), 0, s, tree, desc, n, cap, nidLevel, nodeId, wordId, (int*)nullptr);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

int launch_voc_transform_bow(const VocTree& tree, const double* weight, const uint32_t* desc, const int* n, int cap, int maxN, int B, int nidLevel, int* nodeId, int* wordId, int* leafId,
                             int* bowWord, double* bowValue, int* nWords, hipStream_t s) {
    int sortLen = 1; while (sortLen < maxN) sortLen <<= 1;
    hipLaunchKernelGGL(k_voc_transform<true>, dim3(divup(maxN, VT_NT), B), dim3(VT_NT), 0, s, tree, desc, n, cap, nidLevel, nodeId, wordId, leafId);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bow_vector, dim3(B), dim3(BV_NT), (size_t)sortLen * sizeof(unsigned long long), s, weight, n, cap, sortLen, wordId, leafId, bowWord, bowValue, nWords);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
