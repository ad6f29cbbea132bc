// DynaDetect engine, flow-mask stage (DD:1163-1367): the tail's own stage for one frame and FlowMaskBatch for one frame of every stream of a k-means group.
#include <algorithm>
#include <cstring>
#include "dyna.hpp"
#include "host/rng.hpp"

namespace sind {

// ---- DD:1163-1367: sample weights -> PROSAC pairs -> homography -> residual -> Otsu / Triangle thresholds -> masks
// Three parts: the host part up to the homography (flow_masks_homography), the GPU part (flow_masks_gpu, or FlowMaskBatch for one frame of every stream of a
// k-means group) and the part that turns the results into the two masks and the debug fields (flow_masks_result / flow_masks_ready).
int DynaTail::flow_masks(const float* U, const float* V, BitImg& low, BitImg& high, const float* gridFlowPre) {
    double Hm[9];
    SIND_TRY(flow_masks_homography(U, V, gridFlowPre, Hm));
    SIND_TRY(flow_masks_gpu(U, V, Hm));
    const size_t res_off = ((size_t)2 * N + 15) / 16 * 16;
    flow_masks_result(reinterpret_cast<const int*>(h_ab.p + res_off));
    const double tq = tick_ms();
    low = BitImg::from_u8(h_ab.p, W, H, W); high = BitImg::from_u8((h_ab.p + N), W, H, W);
    t_fine[23] += tick_ms() - tq;
    if (keep_debug) { dbg.maskLow.assign(h_ab.p, h_ab.p + N); dbg.maskHigh.assign((h_ab.p + N), (h_ab.p + N) + N); }
    return SIND_OK;
}
// masks that the batched stage made (bit-packed already): nothing to pack on the host
void DynaTail::flow_masks_ready(const FlowMasksReady& fm, BitImg& low, BitImg& high) {
    flow_masks_result(fm.res);
    const size_t words = (size_t)H * (W / 64);
    low.create(W, H); high.create(W, H);
    std::memcpy(low.d.data(), fm.low, words * 8); std::memcpy(high.d.data(), fm.high, words * 8);
    if (keep_debug) { dbg.maskLow.resize(N); low.to_u8(dbg.maskLow.data(), W, 128); dbg.maskHigh.resize(N); high.to_u8(dbg.maskHigh.data(), W, 255); }
}
void DynaTail::flow_masks_result(const int* hh) {
    float f[5]; std::memcpy(&f[0], hh + 256, 4); std::memcpy(&f[1], hh + 257, 16);
    dbg.maxError = f[0]; dbg.thr_low = f[1]; dbg.thr_high = f[2]; dbg.otsu = f[3]; dbg.triangle = f[4];
    std::copy(hh, hh + 256, dbg.hist);
}
int DynaTail::flow_masks_homography(const float* U, const float* V, const float* gridFlowPre, double Hm[9]) {
    const int numCluster = KM_K;
    const int gx = (W - 1) / 10, gy = (H - 1) / 10;
    const float* gridFlow = gridFlowPre;                      // the pipeline gathers the sample grid of all frames right after the dense flow
    if (!gridFlow) {
        SIND_TRY(launch_gather_grid(stream, U, V, grid_d.p, W, H, 10));
        HIP_TRY(hipMemcpyAsync(h_grid.p, grid_d.p, (size_t)2 * gx * gy * sizeof(float), hipMemcpyDeviceToHost, stream));
        gridFlow = h_grid.p;
    }
    double tq = tick_ms();
    #define QLAP(i) { const double t_ = tick_ms(); t_fine[i] += t_ - tq; tq = t_; }
    // previous-frame dynamic ratio per cluster (DD:1169-1177)
    std::vector<float> clusterWeight(numCluster, 0.0f);
    for (int i = 1; i < numCluster; i++) clusterWeight[i] = (float)lastDyn[i] / (float)(lastCnt[i] + 1.0f);       // counts of the previous frame's labels (see process())
    struct PW { int x, y; float weight; };
    std::vector<PW> pts; pts.reserve((size_t)gx * gy);
    CvRng rng(12345);
    for (int row = 10; row < H; row += 10) for (int col = 10; col < W; col += 10) {
        const float randomd = (float)rng.gaussian(0.5);
        const uint8_t dl = dynaLast[(size_t)row * W + col];
        if (dl < 20) pts.push_back({col, row, randomd + 1.0f});
        else if ((unsigned)(dl - 20) <= 230 - 20) { const int label = labelLast[(size_t)row * W + col]; pts.push_back({col, row, randomd + 1.2f * (1.0f - clusterWeight[label])}); }
        else pts.push_back({col, row, randomd + 0.4f});
    }
    QLAP(20)
    std::sort(pts.begin(), pts.end(), [](const PW& a, const PW& b) { return a.weight > b.weight; });
    if (!gridFlowPre) HIP_TRY(sind_stream_wait(stream));
    QLAP(21)
    std::vector<Pt2f> in, inLast;
    for (const PW& p : pts) {
        const int gi = (p.y / 10 - 1) * gx + (p.x / 10 - 1);
        const float ptCol = (float)p.x, ptRow = (float)p.y, fxv = gridFlow[2 * gi], fyv = gridFlow[2 * gi + 1];
        const int r = (int)(ptRow - fyv), c = (int)(ptCol - fxv);
        if ((unsigned)r <= (unsigned)H && (unsigned)c <= (unsigned)W) { in.push_back({ptCol, ptRow}); inLast.push_back({ptCol - fxv, ptRow - fyv}); }
    }
    tq = tick_ms();
    find_homography_rho(in, inLast, Hm);
    QLAP(22)
    #undef QLAP
    dbg.nPairs = (int)in.size(); std::copy(Hm, Hm + 9, dbg.H);
    return SIND_OK;
}
int DynaTail::flow_masks_gpu(const float* U, const float* V, const double Hm[9]) {
    // working histogram hist_d[0..256] (+ maximum): zero whenever the previous frame's threshold kernel completed (it clears what it read); a frame that
    // failed in between leaves it unknown, hence the flag
    SIND_TRY(launch_residual(stream, U, V, Hm, mag.p, (unsigned*)(hist_d.p + 256), hist_d.p, magu8.p, W, H, hist_clean));
    hist_clean = false;
    // thresholds (Otsu / triangle + the clamping of DD:1309-1367) and the two masks on the device: one host round trip for the stage
    // result block (histogram, maximum, four thresholds) right behind the two masks: it travels with them (a copy of 1 KB of its own was a blit kernel and a launch per frame)
    const size_t res_off = ((size_t)2 * N + 15) / 16 * 16;
    int* res = reinterpret_cast<int*>(low_d.p + res_off);
    SIND_TRY(launch_flow_thresholds_and_masks(stream, hist_d.p, W, H, res, magu8.p, low_d.p, (low_d.p + N)));
    HIP_TRY(hipMemcpyAsync(h_ab.p, low_d.p, res_off + 261 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(sind_stream_wait(stream));
    hist_clean = true;
    return SIND_OK;
}

// ---- the GPU part of the flow-mask stage for one frame of every stream of a k-means group (see dyna.hpp)
int FlowMaskBatch::init(const DynaConfig& c, int cap_, hipStream_t s) {
    cfg = c; W = c.W; H = c.H; cap = cap_; stream = s; slot_words = flow_mask_slot_words(W, H);
    if (W % 64 != 0) { sind_set_error("FlowMaskBatch: width must be a multiple of 64 (got %d)", W); return SIND_E_ARG; }
    SIND_TRY(recs_h.alloc(cap)); SIND_TRY(recs_d.alloc(cap)); SIND_TRY(out_d.alloc(slot_words * cap)); SIND_TRY(out_h.alloc(slot_words * cap));
    tails.assign(cap, nullptr);
    if (!done) HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    return SIND_OK;
}
FlowMaskBatch::~FlowMaskBatch() { if (done) (void)hipEventDestroy(done); }
int FlowMaskBatch::set(int b, DynaTail* tail, const float* U, const float* V, const double Hm[9]) {
    if (b < 0 || b >= cap || !tail) { sind_set_error("FlowMaskBatch::set: slot %d outside [0,%d)", b, cap); return SIND_E_ARG; }
    FlowMaskRec& R = recs_h.p[b];
    R.U = U; R.V = V; std::copy(Hm, Hm + 9, R.H); R.mag = tail->mag.p; R.magu8 = tail->magu8.p; R.hist = tail->hist_d.p; R.out = out_d.p + slot_words * b;
    tails[b] = tail;
    return SIND_OK;
}
int FlowMaskBatch::enqueue(int n) {
    if (n < 1 || n > cap) { sind_set_error("FlowMaskBatch::enqueue: %d frames (capacity %d)", n, cap); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(cfg.device));
    // a working histogram is zero whenever the threshold kernel that read it last completed; a frame that failed in between leaves it unknown
    for (int b = 0; b < n; b++) { if (!tails[b]->hist_clean) HIP_TRY(hipMemsetAsync(tails[b]->hist_d.p, 0, 257 * sizeof(int), stream)); tails[b]->hist_clean = false; }
    HIP_TRY(hipMemcpyAsync(recs_d.p, recs_h.p, (size_t)n * sizeof(FlowMaskRec), hipMemcpyHostToDevice, stream));
    SIND_TRY(launch_flow_masks_frames(stream, recs_d.p, recs_h.p, n, cap, W, H));
    HIP_TRY(hipMemcpyAsync(out_h.p, out_d.p, slot_words * n * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(done, stream));
    pending = n;
    return SIND_OK;
}
int FlowMaskBatch::wait() {
    if (pending < 1) { sind_set_error("FlowMaskBatch::wait: nothing was enqueued"); return SIND_E_STATE; }
    HIP_TRY(sind_event_wait(done));
    for (int b = 0; b < pending; b++) tails[b]->hist_clean = true;
    pending = 0;
    return SIND_OK;
}

}  // namespace sind
