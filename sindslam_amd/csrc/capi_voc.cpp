// C ABI: vocabulary transform (include/sind_hip.h, "sind_voc_*").
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/sind_hip.h"
#include "match.hpp"

struct sind_voc {
    int device = 0, cap = 0, maxB = 0, levels = 0, nNodes = 0; hipStream_t stream = nullptr;
    DevBuf<int> childStart, child, wordId; DevBuf<uint32_t> nodeDesc; DevBuf<uint8_t> stopped;                     // the tree
    Staged<int> n, outNode, outWord; Staged<uint32_t> desc;                                                          // [maxB], [maxB][cap], descriptors as 8 words
    // sind_voc_transform_bow: the nodes' weights as given (FP64); the leaf of every descriptor, the BowVectors and their lengths, on first use
    DevBuf<double> weight; DevBuf<int> outLeaf; Staged<int> bowWord, nWords; Staged<double> bowValue;
};

// what both transforms check before anything is staged: the batch, the counts, the descriptor pointers.  maxN = the largest count
static int check_frames(const char* who, sind_voc* v, const uint8_t* const* desc, const int* n, int B, int cap, int& maxN) {
    if (B > v->maxB) { sind_set_error("%s: B=%d, max_batch %d", who, B, v->maxB); return SIND_E_CAPACITY; }
    maxN = 0;
    for (int b = 0; b < B; b++) {
        if (n[b] < 0 || (n[b] && !desc[b])) { sind_set_error("%s: null array or negative count in frame %d", who, b); return SIND_E_ARG; }
        if (n[b] > cap) { sind_set_error("%s: frame %d has %d descriptors, capacity %d", who, b, n[b], cap); return SIND_E_CAPACITY; }
        maxN = std::max(maxN, n[b]);
    }
    return SIND_OK;
}

// a tree rooted at node 0: CSR in range, every node but the root the child of exactly one node and reachable from the root, every leaf with a word
static const char* tree_fault(const sind_voc_tree* t) {
    const int n = t->n_nodes;
    if (n < 2 || t->levels < 0) return "fewer than two nodes or negative levels";        // the reference's descent reads the root's first child unconditionally
    if (!t->child_start || !t->child || !t->desc || !t->word_id || !t->weight) return "null array";
    if (t->child_start[0] != 0 || t->child_start[n] != n - 1) return "child_start does not span n_nodes - 1 children";
    for (int i = 0; i < n; i++) if (t->child_start[i + 1] < t->child_start[i]) return "child_start decreases";
    std::vector<uint8_t> seen(n, 0);
    for (int j = 0; j < n - 1; j++) {
        const int c = t->child[j];
        if (c < 1 || c >= n) return "child index out of range (the root is nobody's child)";
        if (seen[c]) return "node with two parents";
        seen[c] = 1;
    }
    std::vector<int> stack{0}; int reached = 0;
    while (!stack.empty()) {
        const int i = stack.back(); stack.pop_back(); reached++;
        for (int j = t->child_start[i]; j < t->child_start[i + 1]; j++) stack.push_back(t->child[j]);
    }
    if (reached != n) return "nodes not reachable from the root";
    for (int i = 0; i < n; i++) if (t->child_start[i] == t->child_start[i + 1] && t->word_id[i] < 0) return "leaf without a word";
    return nullptr;
}

extern "C" {

int sind_voc_create(const sind_voc_tree* tree, int cap, int max_batch, int device, sind_voc** out) {
    if (!tree || !out || cap < 1 || max_batch < 1) { sind_set_error("sind_voc_create: bad arguments"); return SIND_E_ARG; }
    if (const char* why = tree_fault(tree)) { sind_set_error("sind_voc_create: not a vocabulary tree: %s", why); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    sind_voc* v = new sind_voc(); v->device = device; v->cap = cap; v->maxB = max_batch; v->levels = tree->levels; v->nNodes = tree->n_nodes;
    const size_t n = tree->n_nodes, nd = (size_t)max_batch * cap;
    std::vector<uint8_t> stopped(n);
    for (size_t i = 0; i < n; i++) stopped[i] = !(tree->weight[i] > 0);                   // TemplatedVocabulary.h:1157 "if(w > 0) // not stopped"
    int r = SIND_OK;
    if ((r = v->childStart.alloc(n + 1)) || (r = v->child.alloc(n - 1)) || (r = v->wordId.alloc(n)) || (r = v->nodeDesc.alloc(n * 8)) || (r = v->stopped.alloc(n)) || (r = v->weight.alloc(n)) || (r = v->n.alloc(max_batch)) ||
        (r = v->outNode.alloc(nd)) || (r = v->outWord.alloc(nd)) || (r = v->desc.alloc(nd * 8))) { delete v; return r; }
    if (hipMemcpy(v->childStart.p, tree->child_start, (n + 1) * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(v->child.p, tree->child, (n - 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->wordId.p, tree->word_id, n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(v->nodeDesc.p, tree->desc, n * 32, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->stopped.p, stopped.data(), n, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(v->weight.p, tree->weight, n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) {
        delete v; sind_set_error("sind_voc_create: uploading the tree failed"); return SIND_E_HIP;
    }
    *out = v; return SIND_OK;
}

int sind_voc_destroy(sind_voc* v) {
    if (!v) return SIND_OK;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    hipStream_t s = v->stream; delete v; if (s) (void)hipStreamDestroy(s);
    return SIND_OK;
}

int sind_voc_transform(sind_voc* v, const uint8_t* const* desc, const int* n, int B, int levelsup, int* const* node_id, int* const* word_id) {
    if (!v || !desc || !n || B < 1) { sind_set_error("sind_voc_transform: bad arguments"); return SIND_E_ARG; }
    int maxN = 0;
    SIND_TRY(check_frames("sind_voc_transform", v, desc, n, B, v->cap, maxN));
    if (!maxN) return SIND_OK;
    HIP_TRY(hipSetDevice(v->device));
    const size_t cap = v->cap, nd = (size_t)B * cap;
    for (int b = 0; b < B; b++) { v->n.h[b] = n[b]; if (n[b]) std::memcpy(&v->desc.h[b * cap * 8], desc[b], (size_t)n[b] * 32); }
    hipStream_t s = v->stream;
    SIND_TRY(v->n.up(B, s)); SIND_TRY(v->desc.up(nd * 8, s));
    const sind::VocTree tr{v->nNodes, v->childStart.p, v->child.p, v->nodeDesc.p, v->wordId.p, v->stopped.p};
    SIND_TRY(sind::launch_voc_transform(tr, v->desc.d.p, v->n.d.p, v->cap, maxN, B, v->levels - levelsup, v->outNode.d.p, v->outWord.d.p, s));
    SIND_TRY(v->outNode.down(nd, s)); SIND_TRY(v->outWord.down(nd, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        if (!n[b]) continue;
        if (node_id && node_id[b]) std::memcpy(node_id[b], &v->outNode.h[b * cap], (size_t)n[b] * 4);
        if (word_id && word_id[b]) std::memcpy(word_id[b], &v->outWord.h[b * cap], (size_t)n[b] * 4);
    }
    return SIND_OK;
}

int sind_voc_transform_bow(sind_voc* v, const uint8_t* const* desc, const int* n, int B, int levelsup, int* const* node_id, int* const* word_id, int* const* bow_word,
                           double* const* bow_value, int* n_words) {
    const char* who = "sind_voc_transform_bow";
    if (!v || !desc || !n || B < 1 || !bow_word || !bow_value || !n_words) { sind_set_error("%s: bad arguments", who); return SIND_E_ARG; }
    int maxN = 0;
    SIND_TRY(check_frames(who, v, desc, n, B, std::min(v->cap, BOW_MAX_KEYS), maxN));
    for (int b = 0; b < B; b++) if (n[b] && (!bow_word[b] || !bow_value[b])) { sind_set_error("%s: null array or negative count in frame %d", who, b); return SIND_E_ARG; }
    if (!maxN) { for (int b = 0; b < B; b++) n_words[b] = 0; return SIND_OK; }
    HIP_TRY(hipSetDevice(v->device));
    const size_t cap = v->cap, nd = (size_t)B * cap, all = (size_t)v->maxB * cap;
    SIND_TRY(v->outLeaf.alloc(all)); SIND_TRY(v->bowWord.alloc(all)); SIND_TRY(v->bowValue.alloc(all)); SIND_TRY(v->nWords.alloc(v->maxB));
    for (int b = 0; b < B; b++) { v->n.h[b] = n[b]; if (n[b]) std::memcpy(&v->desc.h[b * cap * 8], desc[b], (size_t)n[b] * 32); }
    hipStream_t s = v->stream;
    SIND_TRY(v->n.up(B, s)); SIND_TRY(v->desc.up(nd * 8, s));
    const sind::VocTree tr{v->nNodes, v->childStart.p, v->child.p, v->nodeDesc.p, v->wordId.p, v->stopped.p};
    SIND_TRY(sind::launch_voc_transform_bow(tr, v->weight.p, v->desc.d.p, v->n.d.p, v->cap, maxN, B, v->levels - levelsup, v->outNode.d.p, v->outWord.d.p, v->outLeaf.p, v->bowWord.d.p,
                                            v->bowValue.d.p, v->nWords.d.p, s));
    SIND_TRY(v->outNode.down(nd, s)); SIND_TRY(v->outWord.down(nd, s)); SIND_TRY(v->bowWord.down(nd, s)); SIND_TRY(v->bowValue.down(nd, s)); SIND_TRY(v->nWords.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        const int nw = n[b] ? v->nWords.h[b] : 0;
        n_words[b] = nw;
        if (!n[b]) continue;
        if (node_id && node_id[b]) std::memcpy(node_id[b], &v->outNode.h[b * cap], (size_t)n[b] * 4);
        if (word_id && word_id[b]) std::memcpy(word_id[b], &v->outWord.h[b * cap], (size_t)n[b] * 4);
        std::memcpy(bow_word[b], &v->bowWord.h[b * cap], (size_t)nw * sizeof(int)); std::memcpy(bow_value[b], &v->bowValue.h[b * cap], (size_t)nw * sizeof(double));
    }
    return SIND_OK;
}

}  // extern "C"
