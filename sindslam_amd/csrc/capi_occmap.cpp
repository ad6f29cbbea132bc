// C ABI: occupancy map of the mapping consumer (include/sind_hip.h, "sind_occmap_*").
#include <algorithm>
#include <cmath>
#include <cstring>
#include "../../include/sind_hip.h"
#include "occmap_dev.hpp"

static_assert(sizeof(sind_occmap_stats) == sizeof(sind::OccStats), "the ABI struct is the kernels' struct");
static_assert(sizeof(sind_occmap_tree_stats) == sizeof(sind::OccTreeStats), "the ABI struct is the shared struct");

struct sind_occmap {
    int device = 0, maxVoxels = 0, maxPoints = 0, S = 0, gen = 0; sind::OccParams P{}; hipStream_t stream = nullptr;
    DevBuf<sind::OccSlot> slot; DevBuf<int> fill, touched, pslot, ids, sorted, gap, ctl;
    DevBuf<sind::OccStats> stats; DevBuf<sind::CloudPoint> staging;
    // queries: allocated at first use, then reused
    DevBuf<unsigned long long> occKey; DevBuf<uint32_t> occCol; DevBuf<int> occCount; DevBuf<uint8_t> readBuf;
    // the snapshot tree: the node workspace is allocated at the first tree call (sized from max_voxels) and kept; the outputs grow with the largest tree asked for
    int treeT = 0, treeMaxInner = 0; DevBuf<sind::OccTreeNode> treeNode; DevBuf<int> treeList, treeCtl;
    DevBuf<unsigned long long> treeData; DevBuf<sind::CloudPoint> treeLeaves; DevBuf<uint8_t> treeDepth;
    sind::OccTreeArrays tree() { sind::OccTreeArrays t{}; t.T = treeT; t.maxInner = treeMaxInner; t.node = treeNode.p; t.list = treeList.p; t.ctl = treeCtl.p; return t; }
    std::vector<sind::OccStats> h_stats; std::vector<unsigned long long> h_occKey; std::vector<uint32_t> h_occCol;
    sind::OccArrays arrays() {
        sind::OccArrays a{}; a.S = S; a.limit = S - S / 4; a.maxVoxels = maxVoxels;
        a.slot = slot.p; a.fill = fill.p; a.touched = touched.p; a.pslot = pslot.p;
        a.ids = ids.p; a.sorted = sorted.p; a.gap = gap.p; a.ctl = ctl.p; a.stats = stats.p;
        return a;
    }
};

namespace {

// cloud(b) returns the device pointer of key frame b's points (after queueing whatever upload it needs on the stream)
template <class Cloud> int insert_frames(sind_occmap* h, int B, const int* n, const float* origins, sind_occmap_stats* stats, const char* who, Cloud cloud) {
    hipStream_t s = h->stream;
    SIND_TRY(h->stats.alloc(B)); h->h_stats.resize(B);
    HIP_TRY(hipMemsetAsync(h->stats.p, 0, (size_t)B * sizeof(sind::OccStats), s));
    const sind::OccArrays a = h->arrays();
    for (int b = 0; b < B; b++) {
        const sind::CloudPoint* pts = nullptr;
        SIND_TRY(cloud(b, &pts));
        SIND_TRY(sind::launch_occmap_keyframe(a, h->P, pts, n[b], origins + 3 * b, ++h->gen, b, s));
    }
    int ctl[sind::OCC_NCTL];
    HIP_TRY(hipMemcpyAsync(h->h_stats.data(), h->stats.p, (size_t)B * sizeof(sind::OccStats), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ctl, h->ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                                 // the one wait of the call
    const int failed = ctl[sind::OCC_OVERFLOW] ? ctl[sind::OCC_FAILED] : B;
    for (int b = 0; b < B && stats; b++) { if (b < failed) std::memcpy(stats + b, &h->h_stats[b], sizeof(sind_occmap_stats)); else std::memset(stats + b, 0, sizeof(sind_occmap_stats)); }
    if (failed < B) {
        sind_set_error("%s: key frame %d would take the map beyond max_voxels = %d (%d known); the map holds the key frames before it", who, failed, h->maxVoxels, ctl[sind::OCC_KNOWN]);
        return SIND_E_CAPACITY;
    }
    return SIND_OK;
}

int check_frames(sind_occmap* h, int B, const int* n, int stride, const float* origins, const char* who) {
    for (int b = 0; b < B; b++) {
        if (n[b] < 0 || n[b] > stride) { sind_set_error("%s: cloud %d has n_points %d (stride %d)", who, b, n[b], stride); return SIND_E_ARG; }
        if (!sind::occ_finite(origins[3 * b], origins[3 * b + 1], origins[3 * b + 2])) { sind_set_error("%s: origin %d is not finite", who, b); return SIND_E_ARG; }
        if (n[b] > h->maxPoints) { sind_set_error("%s: cloud %d has %d points, the handle holds %d", who, b, n[b], h->maxPoints); return SIND_E_CAPACITY; }
    }
    return SIND_OK;
}

// The bottom-up half and the call's first wait: the counts.  nListed = the leaves the list will hold.
int tree_counts(sind_occmap* h, int prune, int innerColour, int occupiedOnly, sind_occmap_tree_stats* stats, int* nListed, const char* who) {
    hipStream_t s = h->stream;
    if (!h->treeT) {
        const int T = h->S, maxInner = h->S / 2;                       // the header's rule: the flat table's slots, half of them inner nodes at most
        SIND_TRY(h->treeNode.alloc(T)); SIND_TRY(h->treeList.alloc(maxInner)); SIND_TRY(h->treeCtl.alloc(sind::OCCT_NCTL));
        h->treeT = T; h->treeMaxInner = maxInner;
    }
    SIND_TRY(sind::launch_occmap_tree_up(h->arrays(), h->tree(), h->P, prune != 0, innerColour != 0, s));
    int ctl[sind::OCCT_NCTL];
    HIP_TRY(hipMemcpyAsync(ctl, h->treeCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                                 // wait 1: the counts
    if (ctl[sind::OCCT_OVERFLOW]) {
        sind_set_error("%s: the tree has more than %d inner nodes (half the %d slots that max_voxels = %d gives)", who, h->treeMaxInner, h->treeT, h->maxVoxels);
        return SIND_E_CAPACITY;
    }
    sind_occmap_tree_stats st{}; const int* coll = ctl + sind::OCCT_COLLAPSED;
    st.n_nodes = ctl[sind::OCCT_NNODES]; st.n_leaves = ctl[sind::OCCT_NLEAVES]; st.n_inner = st.n_nodes - st.n_leaves; st.n_occupied_leaves = ctl[sind::OCCT_NOCC];
    for (int d = 1; d < 16; d++) { st.n_pruned += coll[d]; st.leaves_at_depth[d] = coll[d] - 8 * coll[d - 1]; }      // a collapsed node is a leaf unless its parent collapsed too
    st.leaves_at_depth[16] = st.n_leaves + 7 * st.n_pruned - 8 * coll[15];                                             // every collapse turns eight leaves into one
    *stats = st; *nListed = occupiedOnly ? st.n_occupied_leaves : st.n_leaves;
    return SIND_OK;
}

// The top-down half into host arrays of exactly n_nodes records / nListed leaves, and the call's second wait.  data, leaves and depth may each be NULL.
int tree_outputs(sind_occmap* h, int occupiedOnly, const sind_occmap_tree_stats& st, int nListed, uint8_t* data, sind_cloud_point* leaves, uint8_t* depth) {
    if ((!data && !leaves) || !st.n_nodes) return SIND_OK;
    hipStream_t s = h->stream; sind::OccTreeOut o{};
    if (data) { SIND_TRY(h->treeData.alloc(st.n_nodes)); o.data = h->treeData.p; o.capNodes = st.n_nodes; }
    if (leaves) { SIND_TRY(h->treeLeaves.alloc(std::max(nListed, 1))); SIND_TRY(h->treeDepth.alloc(std::max(nListed, 1))); o.leaves = h->treeLeaves.p; o.depth = h->treeDepth.p; o.capLeaves = nListed; }
    SIND_TRY(sind::launch_occmap_tree_down(h->arrays(), h->tree(), h->P, occupiedOnly != 0, o, s));
    if (data) HIP_TRY(hipMemcpyAsync(data, o.data, (size_t)st.n_nodes * 8, hipMemcpyDeviceToHost, s));
    if (leaves && nListed) HIP_TRY(hipMemcpyAsync(leaves, o.leaves, (size_t)nListed * sizeof(sind::CloudPoint), hipMemcpyDeviceToHost, s));
    if (leaves && depth && nListed) HIP_TRY(hipMemcpyAsync(depth, o.depth, (size_t)nListed, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                                 // wait 2: the copies sized by the counts
    return SIND_OK;
}

}  // namespace

extern "C" {

int sind_occmap_create(double resolution, double prob_hit, double prob_miss, double clamp_min, double clamp_max, double occ_thres, int max_voxels, int max_points,
                       int device, sind_occmap** out) {
    const double p[5] = {prob_hit, prob_miss, clamp_min, clamp_max, occ_thres};
    bool ok = out && resolution >= SIND_OCCMAP_MIN_RESOLUTION && resolution <= SIND_OCCMAP_MAX_RESOLUTION && max_voxels >= 1 && max_points >= 1 && clamp_min < clamp_max;
    for (int i = 0; i < 5; i++) ok = ok && p[i] > 0.0 && p[i] < 1.0;
    if (!ok) { sind_set_error("sind_occmap_create: bad arguments (a resolution in [1e-6, 1e6], probabilities inside (0, 1), clamp_min < clamp_max, counts >= 1)"); return SIND_E_ARG; }
    if (max_voxels > (1 << 26) || max_points > (1 << 26)) { sind_set_error("sind_occmap_create: max_voxels and max_points are limited to 2^26"); return SIND_E_CAPACITY; }
    HIP_TRY(hipSetDevice(device));
    sind_occmap* h = new sind_occmap(); h->device = device; h->maxVoxels = max_voxels; h->maxPoints = max_points;
    h->P = sind::occ_params(resolution, p[0], p[1], p[2], p[3], p[4]);
    h->S = 1024; while (h->S < 2 * max_voxels) h->S *= 2;
    const size_t S = h->S, np = max_points; int r = SIND_OK;
    if ((r = h->slot.alloc(S)) || (r = h->fill.alloc(S)) || (r = h->touched.alloc(S)) || (r = h->pslot.alloc(np)) || (r = h->ids.alloc(2 * np)) || (r = h->sorted.alloc(2 * np)) || (r = h->gap.alloc(2 * np)) ||
        (r = h->ctl.alloc(sind::OCC_NCTL)) || (r = h->stats.alloc(8)) || (r = h->staging.alloc(np))) { delete h; return r; }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; sind_set_error("sind_occmap_create: stream creation failed"); return SIND_E_HIP; }
    r = sind_occmap_clear(h);
    if (r != SIND_OK) { sind_occmap_destroy(h); return r; }
    *out = h; return SIND_OK;
}
int sind_occmap_destroy(sind_occmap* h) {
    if (!h) return SIND_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    hipStream_t s = h->stream; delete h; if (s) (void)hipStreamDestroy(s);
    return SIND_OK;
}
int sind_occmap_clear(sind_occmap* h) {
    if (!h) { sind_set_error("sind_occmap_clear: NULL handle"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    SIND_TRY(sind::launch_occmap_clear(h->arrays(), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->gen = 0; return SIND_OK;
}
int sind_occmap_size(sind_occmap* h) {
    if (!h) { sind_set_error("sind_occmap_size: NULL handle"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    int known = 0;
    HIP_TRY(hipMemcpyAsync(&known, h->ctl.p + sind::OCC_KNOWN, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return known;
}

int sind_occmap_insert(sind_occmap* h, int B, const sind_cloud_point* points, int stride, const int* n_points, const float* origins, int inputs_on_device,
                       sind_occmap_stats* stats) {
    if (!h || B < 1 || !n_points || !origins || stride < 0) { sind_set_error("sind_occmap_insert: bad arguments (B=%d)", B); return SIND_E_ARG; }
    SIND_TRY(check_frames(h, B, n_points, stride, origins, "sind_occmap_insert"));
    for (int b = 0; b < B; b++) if (n_points[b] > 0 && !points) { sind_set_error("sind_occmap_insert: points is NULL"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    return insert_frames(h, B, n_points, origins, stats, "sind_occmap_insert", [&](int b, const sind::CloudPoint** pts) {
        const sind::CloudPoint* src = points ? reinterpret_cast<const sind::CloudPoint*>(points) + (size_t)b * stride : nullptr;
        if (inputs_on_device || !n_points[b]) { *pts = inputs_on_device ? src : h->staging.p; return SIND_OK; }
        // one staging cloud: the copy of key frame b is ordered on the stream behind the kernels of key frame b - 1
        HIP_TRY(hipMemcpyAsync(h->staging.p, src, (size_t)n_points[b] * sizeof(sind::CloudPoint), hipMemcpyHostToDevice, h->stream));
        *pts = h->staging.p; return SIND_OK;
    });
}

int sind_occmap_insert_generated(sind_occmap* h, sind_cloud* cloud, int B, const float* origins, sind_occmap_stats* stats) {
    if (!h || !cloud || B < 1 || !origins) { sind_set_error("sind_occmap_insert_generated: bad arguments (B=%d)", B); return SIND_E_ARG; }
    const sind::CloudResident c = sind::cloud_resident(cloud);
    if (c.device != h->device) { sind_set_error("sind_occmap_insert_generated: the cloud handle lives on device %d, the map on %d", c.device, h->device); return SIND_E_ARG; }
    if (B > c.lastB) { sind_set_error("sind_occmap_insert_generated: asks for %d clouds, the last sind_cloud_generate left %d", B, c.lastB); return SIND_E_STATE; }
    SIND_TRY(check_frames(h, B, c.n, c.stride, origins, "sind_occmap_insert_generated"));
    HIP_TRY(hipSetDevice(h->device));
    return insert_frames(h, B, c.n, origins, stats, "sind_occmap_insert_generated", [&](int b, const sind::CloudPoint** pts) { *pts = c.pts + (size_t)b * c.stride; return SIND_OK; });
}

int sind_occmap_occupied(sind_occmap* h, sind_cloud_point* out, int cap, int* n_out) {
    if (!h || !n_out || (out && cap < 0)) { sind_set_error("sind_occmap_occupied: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream; int n = 0;
    SIND_TRY(h->occCount.alloc(1));
    if (out) { SIND_TRY(h->occKey.alloc(h->maxVoxels)); SIND_TRY(h->occCol.alloc(h->maxVoxels)); }
    SIND_TRY(sind::launch_occmap_occupied(h->arrays(), h->P.occLog, h->occKey.p, h->occCol.p, out ? h->maxVoxels : 0, h->occCount.p, s));
    HIP_TRY(hipMemcpyAsync(&n, h->occCount.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                                 // wait 1: the count
    *n_out = n;
    if (!out) return SIND_OK;
    if (n > cap) { sind_set_error("sind_occmap_occupied: %d occupied voxels, capacity %d", n, cap); return SIND_E_CAPACITY; }
    if (!n) return SIND_OK;
    h->h_occKey.resize(n); h->h_occCol.resize(n);
    HIP_TRY(hipMemcpyAsync(h->h_occKey.data(), h->occKey.p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h->h_occCol.data(), h->occCol.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                                 // wait 2: the copies sized by it
    // leaf_iterator order: the compaction's order is the slots', which is nobody's; the Morton sort runs here, on the host
    std::vector<std::pair<uint64_t, int>> order(n);
    for (int i = 0; i < n; i++) order[i] = {sind::occ_morton(h->h_occKey[i]), i};
    std::sort(order.begin(), order.end());
    for (int i = 0; i < n; i++) {
        const uint64_t k = h->h_occKey[order[i].second]; const uint32_t c = h->h_occCol[order[i].second];
        out[i].x = (float)sind::occ_coord(h->P, (int)(k & 0xffff)); out[i].y = (float)sind::occ_coord(h->P, (int)((k >> 16) & 0xffff)); out[i].z = (float)sind::occ_coord(h->P, (int)((k >> 32) & 0xffff));
        out[i].r = c & 255; out[i].g = (c >> 8) & 255; out[i].b = (c >> 16) & 255; out[i].a = 0;
    }
    return SIND_OK;
}

int sind_occmap_read(sind_occmap* h, const uint16_t* keys, int n, uint8_t* known, uint32_t* logodds, uint8_t* rgb) {
    if (!h || n < 0 || (n > 0 && (!keys || !known || !logodds || !rgb))) { sind_set_error("sind_occmap_read: bad arguments"); return SIND_E_ARG; }
    if (!n) return SIND_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream; const size_t N = n;
    SIND_TRY(h->readBuf.alloc(N * 16));                               // logodds [n] u32 | keys [n][3] u16 | rgb [n][3] | known [n]
    uint32_t* dLog = reinterpret_cast<uint32_t*>(h->readBuf.p); uint16_t* dKeys = reinterpret_cast<uint16_t*>(h->readBuf.p + 4 * N);
    uint8_t* dRgb = h->readBuf.p + 10 * N; uint8_t* dKnown = h->readBuf.p + 13 * N;
    HIP_TRY(hipMemcpyAsync(dKeys, keys, 6 * N, hipMemcpyHostToDevice, s));
    SIND_TRY(sind::launch_occmap_read(h->arrays(), dKeys, n, dKnown, dLog, dRgb, s));
    HIP_TRY(hipMemcpyAsync(logodds, dLog, 4 * N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(rgb, dRgb, 3 * N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(known, dKnown, N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SIND_OK;
}

int sind_occmap_tree(sind_occmap* h, int prune, int inner_colour, int occupied_only, uint8_t* data, size_t cap_bytes, sind_cloud_point* leaves, uint8_t* leaf_depth,
                     int cap_leaves, int* n_leaves_out, sind_occmap_tree_stats* stats) {
    if (!h || !stats || (leaves && cap_leaves < 0) || (leaf_depth && !leaves)) { sind_set_error("sind_occmap_tree: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    int nListed = 0;
    SIND_TRY(tree_counts(h, prune, inner_colour, occupied_only, stats, &nListed, "sind_occmap_tree"));
    if (n_leaves_out) *n_leaves_out = nListed;
    if (data && (size_t)stats->n_nodes * 8 > cap_bytes) { sind_set_error("sind_occmap_tree: the stream has %zu bytes, capacity %zu", (size_t)stats->n_nodes * 8, cap_bytes); return SIND_E_CAPACITY; }
    if (leaves && nListed > cap_leaves) { sind_set_error("sind_occmap_tree: %d leaves, capacity %d", nListed, cap_leaves); return SIND_E_CAPACITY; }
    return tree_outputs(h, occupied_only, *stats, nListed, data, leaves, leaf_depth);
}

int sind_occmap_write_ot(sind_occmap* h, int prune, int inner_colour, const char* path) {
    if (!h || !path) { sind_set_error("sind_occmap_write_ot: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    sind_occmap_tree_stats st; int nListed = 0;
    SIND_TRY(tree_counts(h, prune, inner_colour, 0, &st, &nListed, "sind_occmap_write_ot"));
    std::vector<uint8_t> data((size_t)st.n_nodes * 8);
    SIND_TRY(tree_outputs(h, 0, st, nListed, data.data(), nullptr, nullptr));
    if (!sind::occ_tree_write_file(path, sind::occ_tree_ot_header(st.n_nodes, h->P.res), data.data(), data.size())) { sind_set_error("sind_occmap_write_ot: cannot write %s", path); return SIND_E_ARG; }
    return SIND_OK;
}

}  // extern "C"
