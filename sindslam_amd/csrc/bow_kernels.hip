// The feature-vector half of Frame::ComputeBoW / KeyFrame::ComputeBoW on the GPU: TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)
// (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259) for every descriptor of B frames, with FORB::distance = Hamming distance.
// One thread per descriptor, its 32 bytes in registers; the tree (CSR children, 32 B per node) is read through the caches: the top levels are shared
// by every thread, and a descent touches levels * k nodes.  Integer work only, so the result is the reference's bit for bit.
//   descent   from the root, at every level the child of smallest distance, strict '<' in the children's order (the first child wins a tie), until a
//             childless node; word_id = that leaf's word
//   node_id   the node passed at level (levels - levelsup); 0 when that level is <= 0; the leaf itself when the path ends above that level (the
//             reference leaves nid uninitialised there); -1 when the word is stopped, !(weight > 0), which keeps the feature out of mFeatVec (:1157-1161)
#include "match.hpp"
#include "match_device.hpp"

namespace sind {

#define VT_NT 256

__global__ __launch_bounds__(VT_NT) void k_voc_transform(VocTree tr, const uint32_t* desc, const int* n, int cap, int nidLevel, int* nodeId, int* wordId) {
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
}

int launch_voc_transform(const VocTree& tree, const uint32_t* desc, const int* n, int cap, int maxN, int B, int nidLevel, int* nodeId, int* wordId, hipStream_t s) {
    hipLaunchKernelGGL(k_voc_transform, dim3(divup(maxN, VT_NT), B), dim3(VT_NT), 0, s, tree, desc, n, cap, nidLevel, nodeId, wordId);
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
