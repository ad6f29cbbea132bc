// DynaDetect engine, SegByKmeans (DD:315-420): the one statement of the k-means launch chain (KmChain), the tail's one-frame stage around it
// (HIP graph) and KMeansBatch for one frame of every stream.
#include <cstring>
#include "dyna.hpp"

namespace sind {

// ---- DD:315-420: 4-level k-means, K = 12, criteria (EPS+COUNT, 4, 0.07), KMEANS_USE_INITIAL_LABELS.
// The whole loop is enqueued without a host round trip: the centre step, empty-cluster repair and the stop test of cv::kmeans
// run in k_km_update (one workgroup) on the device; one D2H of the level-0 state + labels at the end.
int KmChain::init(int W_, int H_, int cap_) {
    W = W_; H = H_; N = W * H; cap = cap_;
    const size_t B = (size_t)cap;
    for (int l = 1; l < 4; l++) SIND_TRY(dpyr[l].alloc(((size_t)N >> (2 * l)) * B));
    for (int l = 0; l < 4; l++) SIND_TRY(lab[l].alloc(((size_t)N >> (2 * l)) * B));
    SIND_TRY(px.alloc((size_t)N * B)); SIND_TRY(py.alloc((size_t)N * B)); SIND_TRY(pz.alloc((size_t)N * B));
    SIND_TRY(comp.alloc((size_t)3 * N * B + 8));       // + 8: k_km_seqsum's window loads may touch up to 7 floats behind the last run
    SIND_TRY(seg.alloc((size_t)KM_SEG_WORDS * B));     // count table, totals row, the 36 sums
    SIND_TRY(labPrev8.alloc((size_t)N * B)); SIND_TRY(lab8.alloc((size_t)N * B)); SIND_TRY(kstate.alloc(4 * B));
    return SIND_OK;
}
int KmChain::enqueue(hipStream_t s, const DynaConfig& cfg, const KmFuse& fuse, const uint16_t* depth_base, size_t depth_stride, int B, const int* use_prev_dev, bool use_prev_host) const {
    if (B < 1 || B > cap) { sind_set_error("KmChain::enqueue: batch %d outside [1,%d]", B, cap); return SIND_E_ARG; }
    const float scales[4] = {1.0f, 0.5f, 0.25f, 0.125f};
    const uint16_t* dl[4] = {depth_base, dpyr[1].p, dpyr[2].p, dpyr[3].p};
    const size_t ds[4] = {depth_stride, (size_t)N >> 2, (size_t)N >> 4, (size_t)N >> 6};
    for (int l = 1; l < 4; l++) SIND_TRY(launch_depth_half(s, dl[l - 1], dpyr[l].p, W >> l, H >> l, B, ds[l - 1], ds[l]));
    for (int level = 3; level >= 0; level--) {
        const int hp = (int)(H * scales[level]), wp = (int)(W * scales[level]), n = hp * wp; const size_t ls = (size_t)N >> (2 * level);
        SIND_TRY(launch_points(s, dl[level], px.p, py.p, pz.p, wp, hp, scales[level], cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.depthScale, B, ds[level], N));
        if (level == 3) {
            if (use_prev_dev || !use_prev_host) SIND_TRY(launch_labels_grid(s, lab[3].p, wp, hp, B, ls, use_prev_dev));
            if (use_prev_dev || use_prev_host) SIND_TRY(launch_labels_resize_u8(s, labPrev8.p, lab[3].p, W, H, wp, hp, B, N, ls, use_prev_dev));
        } else SIND_TRY(launch_labels_resize_i32(s, lab[level + 1].p, lab[level].p, wp / 2, hp / 2, wp, hp, B, (size_t)N >> (2 * (level + 1)), ls));
        SIND_TRY(launch_kmeans_level(s, fuse, px.p, py.p, pz.p, lab[level].p, n, seg.p, comp.p, kstate.p + level, 4, 0.07 * 0.07, B, N, ls, KM_SEG_WORDS, (size_t)3 * N, 4));
    }
    SIND_TRY(launch_labels_to_u8(s, lab[0].p, lab8.p, N, B, N, N));
    return SIND_OK;
}

// ---- one frame on the tail's stream.  The ~50 launches of a frame's k-means are recorded once per tail as a HIP graph (two variants: grid labels for the very first
// frame, previous-frame labels afterwards) and replayed with one hipGraphLaunch: the packets reach the queue in one go instead of
// one host submission per kernel.  The graph reads the depth frame from a fixed per-tail buffer.
int DynaTail::kmeans(const uint16_t* depth_dev, std::vector<uint8_t>& label8, float centers[KM_K][3], int counts[KM_K]) {
    if (kmLabelLastAny) { std::memcpy(h_lab8.p, kmLabelLast.data(), N); HIP_TRY(hipMemcpyAsync(km.labPrev8.p, h_lab8.p, N, hipMemcpyHostToDevice, stream)); }
    bool graphed = false;
    if (!kmGraphBroken) {
        const int v = kmLabelLastAny ? 1 : 0;
        if (!kmGraph[v]) {                       // record once; any failure here only means "launch kernel by kernel from now on" (still the GPU path)
            hipGraph_t g = nullptr;
            if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                const int rc = km.enqueue(stream, cfg, km_fuse, depth_fix.p, N, 1, nullptr, v != 0);
                const hipError_t ec = hipStreamEndCapture(stream, &g);
                if (rc != SIND_OK || ec != hipSuccess || hipGraphInstantiate(&kmGraph[v], g, nullptr, nullptr, 0) != hipSuccess) { kmGraph[v] = nullptr; kmGraphBroken = true; }
                if (g) (void)hipGraphDestroy(g);
            } else kmGraphBroken = true;
            if (kmGraphBroken) { const hipError_t le = hipGetLastError(); fprintf(stderr, "[sind] k-means HIP graph unavailable (%s); launching the chain kernel by kernel\n", hipGetErrorString(le)); }
        }
        if (!kmGraphBroken) {
            HIP_TRY(hipMemcpyAsync(depth_fix.p, depth_dev, (size_t)N * sizeof(uint16_t), hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipGraphLaunch(kmGraph[v], stream));
            graphed = true;
        }
    }
    if (!graphed) SIND_TRY(km.enqueue(stream, cfg, km_fuse, depth_dev, N, 1, nullptr, kmLabelLastAny));
    label8.resize(N);
    HIP_TRY(hipMemcpyAsync(h_kstate.p, km.kstate.p, 4 * sizeof(KmState), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_ab.p, km.lab8.p, N, hipMemcpyDeviceToHost, stream));
    HIP_TRY(sind_stream_wait(stream));
    const KmState* st = h_kstate.p; std::memcpy(label8.data(), h_ab.p, N);
    std::memcpy(centers, st[0].ctr, sizeof(st[0].ctr)); std::memcpy(counts, st[0].cnt, sizeof(st[0].cnt));
    return SIND_OK;
}

// ---- the same chain for one frame of every stream (see dyna.hpp)
int KMeansBatch::init(const DynaConfig& c, int maxB_, hipStream_t s) {
    cfg = c; N = c.W * c.H; maxB = maxB_; stream = s;
    const size_t B = (size_t)maxB;
    SIND_TRY(km.init(c.W, c.H, maxB)); SIND_TRY(use_prev_d.alloc(B));
    SIND_TRY(h_prev.alloc((size_t)N * B)); SIND_TRY(h_lab8.alloc((size_t)N * B)); SIND_TRY(h_state.alloc(4 * B)); SIND_TRY(h_use_prev.alloc(B));
    res.resize(maxB);
    return SIND_OK;
}
int KMeansBatch::run(const uint16_t* depth_base, size_t depth_stride, int B, const uint8_t* const* prev) {
    if (B < 1 || B > maxB) { sind_set_error("KMeansBatch::run: batch %d outside [1,%d]", B, maxB); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(cfg.device));
    bool any_prev = false;
    for (int b = 0; b < B; b++) { h_use_prev.p[b] = prev[b] ? 1 : 0; if (prev[b]) { std::memcpy(h_prev.p + (size_t)N * b, prev[b], N); any_prev = true; } }
    HIP_TRY(hipMemcpyAsync(use_prev_d.p, h_use_prev.p, B * sizeof(int), hipMemcpyHostToDevice, stream));
    if (any_prev) HIP_TRY(hipMemcpyAsync(km.labPrev8.p, h_prev.p, (size_t)N * B, hipMemcpyHostToDevice, stream));
    SIND_TRY(km.enqueue(stream, cfg, km_fuse, depth_base, depth_stride, B, use_prev_d.p, false));
    HIP_TRY(hipMemcpyAsync(h_state.p, km.kstate.p, (size_t)4 * B * sizeof(KmState), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_lab8.p, km.lab8.p, (size_t)N * B, hipMemcpyDeviceToHost, stream));
    HIP_TRY(sind_stream_wait(stream));
    for (int b = 0; b < B; b++) { const KmState& st = h_state.p[4 * b];
        res[b].label8 = h_lab8.p + (size_t)N * b; std::memcpy(res[b].centers, st.ctr, sizeof(st.ctr)); std::memcpy(res[b].counts, st.cnt, sizeof(st.cnt)); }
    return SIND_OK;
}

}  // namespace sind
