// DynaDetect engine: orchestration of the HIP stages and the serial host stages of one stream's tail.
// Reference walk: ORB_SLAM2/src/DynaDetect.cc DetectDynaArea :1377-1666, DetectDynaByDenseOpticalFLow :1023-1374,
// SegByKmeans :315-420, CalOccluded :429-642, SegAndMergeV2 :653-1018, cal_hist :1685-1739.
// Per-pixel work runs in flow_prep.hip / flow_mask.hip / depth_kmeans.hip / depth_edges.hip / depth_rag.hip; contour / graph / flood-fill logic is serial, tiny and
// order-defined and runs on bit-packed masks on the host (DESIGN.md "host stages").  No CPU fallback exists for any
// device stage: every launch error is returned to the caller.
// This file: init, reset, the state blob, process* / depth_stage* / flow_stage and the fusion.  The stages themselves: dyna_flow_masks.cpp, dyna_kmeans.cpp,
// dyna_occluded.cpp, dyna_seg_merge.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "dyna.hpp"
#include "host/statehash.hpp"

namespace sind {

// ======================================================================================================= tail
int DynaTail::init(const DynaConfig& c, hipStream_t s) {
    cfg = c; stream = s; W = c.W; H = c.H; N = W * H;
    invDepthScale = 1.0f / cfg.depthScale; zInvalidFrom = z_invalid_from(cfg.depthScale);
    if (W % 64 != 0 || W % 8 != 0 || H % 8 != 0) { sind_set_error("DynaTail: width must be a multiple of 64 and height of 8 (got %dx%d)", W, H); return SIND_E_ARG; }
    reset();
    SIND_TRY(km.init(W, H, 1)); SIND_TRY(occ.init(cfg, 1));       // the k-means chain's and the CalOccluded front's workspaces for one frame (dyna_kmeans.cpp, dyna_occluded.cpp)
    SIND_TRY(depthN.alloc(N)); SIND_TRY(occ2_d.alloc(N));
    SIND_TRY(magu8.alloc(N)); SIND_TRY(low_d.alloc(((size_t)2 * N + 15) / 16 * 16 + 1088)); SIND_TRY(mag.alloc(N));       // low_d: low mask, high mask, then (16-byte aligned) the thresholds' 261-word result block: ONE D2H for the stage
    SIND_TRY(h_grid.alloc((size_t)2 * ((W - 1) / 10) * ((H - 1) / 10) + 2)); SIND_TRY(h_hist.alloc(261)); SIND_TRY(h_ab.alloc(((size_t)2 * N + 15) / 16 * 16 + 1088)); SIND_TRY(h_lab8.alloc(N));
    SIND_TRY(h_kstate.alloc(4)); SIND_TRY(h_blocks.alloc((size_t)(W / 16) * (H / 16)));
    { // RAG workspaces for up to 64 pieces up front: a later (re)allocation synchronises the whole device, i.e. waits for the
      // flow solver of the next step when tails and dense flow overlap
      const size_t cap = 64, pw = (size_t)H * (W / 64), nr = 3 * cap * cap + cap + cap * 256;
      SIND_TRY(h_planes.alloc(3 * cap * pw)); SIND_TRY(planes_d.alloc(3 * cap * pw)); SIND_TRY(h_rag.alloc(nr)); SIND_TRY(rag_d.alloc(nr)); }
    SIND_TRY(depth_fix.alloc(N));
    SIND_TRY(hist_d.alloc(264 + 261));       // working block [0..256] = residual histogram + maximum (float bits); result block at 264: the same + thresholds lo, hi, otsu, triangle (floats)
    SIND_TRY(grid_d.alloc((size_t)2 * ((W - 1) / 10) * ((H - 1) / 10) + 2));
    // every kernel operand of the tail must exist before the first launch (a missing workspace would be a wild device write)
    const void* ws[] = {km.dpyr[1].p, km.dpyr[2].p, km.dpyr[3].p, km.lab[0].p, km.lab[1].p, km.lab[2].p, km.lab[3].p, occ.filt.p, km.px.p, km.py.p, km.pz.p, km.lab8.p, km.labPrev8.p,
                        occ.edge.p, occ.edgeTmp.p, occ.total.p, depthN.p, occ2_d.p, magu8.p, low_d.p, mag.p, km.seg.p, km.comp.p, occ.umax.p, h_grid.p, h_hist.p, h_ab.p, h_lab8.p, h_kstate.p,
                        h_blocks.p, h_planes.p, planes_d.p, h_rag.p, rag_d.p, km.kstate.p, depth_fix.p, hist_d.p, grid_d.p, occ.blocks.p};
    for (const void* q : ws) if (!q) { sind_set_error("DynaTail::init: a workspace was not allocated"); return SIND_E_STATE; }
    return SIND_OK;
}
void DynaTail::reset() { dynaLast.assign(N, 0); labelLast.assign(N, 0); kmLabelLast.assign(N, 0); highLast.create(W, H); kmLabelLastAny = false; std::memset(lastCnt, 0, sizeof(lastCnt)); std::memset(lastDyn, 0, sizeof(lastDyn)); }

void DynaTail::save_state(uint8_t* buf, bool flow_half, bool depth_half) const {
    uint8_t* q = buf;
    if (flow_half) { std::memcpy(q, dynaLast.data(), N); std::memcpy(q + N, labelLast.data(), N); highLast.to_u8(q + 2 * (size_t)N, W, 255);
                     std::memcpy(q + 3 * (size_t)N, lastCnt, sizeof(lastCnt)); std::memcpy(q + 3 * (size_t)N + sizeof(lastCnt), lastDyn, sizeof(lastDyn)); }
    q += 3 * (size_t)N + sizeof(lastCnt) + sizeof(lastDyn);
    if (depth_half) { std::memcpy(q, kmLabelLast.data(), N); const int any = kmLabelLastAny ? 1 : 0; std::memcpy(q + N, &any, sizeof(int)); }
}
void DynaTail::load_state(const uint8_t* buf, bool flow_half, bool depth_half) {
    const uint8_t* q = buf;
    if (flow_half) { std::memcpy(dynaLast.data(), q, N); std::memcpy(labelLast.data(), q + N, N); highLast = BitImg::from_u8(q + 2 * (size_t)N, W, H, W);
                     std::memcpy(lastCnt, q + 3 * (size_t)N, sizeof(lastCnt)); std::memcpy(lastDyn, q + 3 * (size_t)N + sizeof(lastCnt), sizeof(lastDyn)); }
    q += 3 * (size_t)N + sizeof(lastCnt) + sizeof(lastDyn);
    if (depth_half) { std::memcpy(kmLabelLast.data(), q, N); int any = 0; std::memcpy(&any, q + N, sizeof(int)); kmLabelLastAny = any != 0; }
}

// ---- DD:1377-1666
int DynaTail::process(const uint16_t* depth_host, const uint16_t* depth_dev, const float* U, const float* V, uint8_t* dyna_out, uint8_t* label_out,
                      const OccResult* pre, DynaTail* depth_half, const KmFrameResult* km, const FlowMasksReady* fm) {
    // same stage order as the reference (flow masks, clustering, fusion); the order also matters for throughput: a pool of tails that
    // all start with the 50-launch k-means chain was measured 20 ms per step slower than one that starts with the host-side pair sorting
    HIP_TRY(hipSetDevice(cfg.device));
    BitImg maskLow, maskHigh; n_frames++;
    { const double t0 = tick_ms(); if (fm) flow_masks_ready(*fm, maskLow, maskHigh); else SIND_TRY(flow_masks(U, V, maskLow, maskHigh, pre ? pre->gridFlow : nullptr)); t_stage[0] += tick_ms() - t0; }
    DepthStageOut d;
    SIND_TRY((depth_half ? depth_half : this)->depth_stage(depth_host, depth_dev, pre, d, km));
    return fuse(maskLow, maskHigh, d, dyna_out, label_out);
}
// the same in two parts around the batched RAG stage (dyna.hpp)
int DynaTail::process_begin(const uint16_t* depth_host, const uint16_t* depth_dev, const float* U, const float* V, const OccResult* pre, DynaTail* depth_half,
                            const KmFrameResult* km, const FlowMasksReady* fm) {
    SIND_TRY(process_begin_inputs(depth_host, depth_dev, U, V, pre, depth_half, km, fm));
    return rag_half()->depth_stage_pieces();
}
// ... and that in two parts around a round's batched piece stage (dyna.hpp): up to the inputs of the piece extraction
int DynaTail::process_begin_inputs(const uint16_t* depth_host, const uint16_t* depth_dev, const float* U, const float* V, const OccResult* pre, DynaTail* depth_half,
                                   const KmFrameResult* km, const FlowMasksReady* fm) {
    HIP_TRY(hipSetDevice(cfg.device));
    n_frames++; pendHalf = depth_half;
    { const double t0 = tick_ms(); if (fm) flow_masks_ready(*fm, pendLow, pendHigh); else SIND_TRY(flow_masks(U, V, pendLow, pendHigh, pre ? pre->gridFlow : nullptr)); t_stage[0] += tick_ms() - t0; }
    pendD = DepthStageOut();
    return rag_half()->depth_stage_inputs(depth_host, depth_dev, pre, pendD, km);
}
int DynaTail::process_end(const int* rag, uint8_t* dyna_out, uint8_t* label_out, const uint8_t* piece_of) {
    HIP_TRY(hipSetDevice(cfg.device));
    if (piece_of) { DynaTail* h = rag_half(); h->segPieceOf.assign(piece_of, piece_of + h->N); }
    SIND_TRY(rag_half()->depth_stage_end(pendD, rag));
    return fuse(pendLow, pendHigh, pendD, dyna_out, label_out);
}

// flow-independent half: k-means (DD:1410-1414), cluster order (DD:1428-1491), CalOccluded (DD:1493), SegAndMerge (DD:1495-1551)
int DynaTail::depth_stage(const uint16_t* depth_host, const uint16_t* depth_dev, const OccResult* pre, DepthStageOut& out, const KmFrameResult* km) {
    SIND_TRY(depth_stage_begin(depth_host, depth_dev, pre, out, km));
    const int* rag = nullptr;
    if (!segAll.empty()) SIND_TRY(rag_own(&rag));
    return depth_stage_end(out, rag);
}
int DynaTail::depth_stage_begin(const uint16_t* depth_host, const uint16_t* depth_dev, const OccResult* pre, DepthStageOut& out, const KmFrameResult* km) {
    SIND_TRY(depth_stage_inputs(depth_host, depth_dev, pre, out, km));
    return depth_stage_pieces();
}
int DynaTail::depth_stage_pieces() {
    const double tk = tick_ms();
    if (!segLabels.empty()) SIND_TRY(seg_pieces(segLabels, segOcc1, segEdge, segDepthHost));
    t_stage[4] += tick_ms() - tk;
    return SIND_OK;
}
int DynaTail::depth_stage_inputs(const uint16_t* depth_host, const uint16_t* depth_dev, const OccResult* pre, DepthStageOut& out, const KmFrameResult* km) {
    HIP_TRY(hipSetDevice(cfg.device));
    double tk = tick_ms();
    #define LAP(i) { const double t_ = tick_ms(); t_stage[i] += t_ - tk; tk = t_; }
    std::vector<uint8_t> label8; float centers[KM_K][3]; int counts[KM_K];
    if (km) { label8.assign(km->label8, km->label8 + N); std::memcpy(centers, km->centers, sizeof(centers)); std::memcpy(counts, km->counts, sizeof(counts)); }
    else SIND_TRY(kmeans(depth_dev, label8, centers, counts));
    if (keep_debug) { dbg.kmeansLabel = label8; std::memcpy(dbg.centers, centers, sizeof(centers)); }
    LAP(1)
    // nearest clusters first (DD:1428-1491)
    float depth_vals[KM_K]; int order[KM_K];
    for (int i = 0; i < KM_K; i++) { depth_vals[i] = centers[i][2]; if (depth_vals[i] < 0.2) depth_vals[i] += 20.0f; order[i] = i; }
    std::stable_sort(order, order + KM_K, [&](int a, int b) { return depth_vals[a] < depth_vals[b]; });
    std::vector<BitImg> labelMask(KM_K); BitImg::split_labels(label8.data(), W, H, W, 0, KM_K, labelMask.data());
    std::vector<BitImg>& allLabels = segLabels; allLabels.clear(); BitImg& labelForSegEdge = segEdge; labelForSegEdge.create(W, H);
    float ratioArea = 0.0f; const float TotalArea = (float)(H * W); int count0 = 0;
    for (int i = 0; i < KM_K; i++) {
        const int idx = order[i]; const int cnt = labelMask[idx].count();
        if (cnt < 60) continue;
        allLabels.push_back(labelMask[idx]);
        const float ratio = (float)cnt * (1.0f / TotalArea); ratioArea += ratio;
        if (count0 <= 5 && ratioArea < 0.6f) { labelForSegEdge |= labelMask[idx]; ++count0; }
    }
    labelForSegEdge = labelForSegEdge.dilated(EllipseElem(7));
    BitImg& occ1 = segOcc1; BitImg& occ2 = segOcc2;
    LAP(2)
    if (pre && pre->ready) { out.totalArea = pre->totalArea; occ1 = pre->occ1; occ2 = pre->occ2; }
    else SIND_TRY(cal_occluded(depth_host, depth_dev, out.totalArea, occ1, occ2));
    LAP(3)
    out.label3.assign(N, 0);
    segAll.clear(); segOnDevice = false; segDepthDev = depth_dev; segDepthHost = depth_host; segPre = pre && pre->ready ? pre : nullptr;
    #undef LAP
    return SIND_OK;
}
int DynaTail::depth_stage_end(DepthStageOut& out, const int* rag) {
    const BitImg& occ1 = segOcc1; const BitImg& occ2 = segOcc2;
    if (!segAll.empty()) {
        if (!rag) { sind_set_error("DynaTail::depth_stage_end: the RAG counters of this frame are missing"); return SIND_E_STATE; }
        const double t0 = tick_ms(); seg_finish(rag, out.label3); t_stage[4] += tick_ms() - t0;
    }
    segAll.clear();
    int maxNum = 0; for (uint8_t v : out.label3) maxNum = std::max<int>(maxNum, v);
    out.maxNum = maxNum; out.ready = true;
    if (keep_debug) { dbg.occ1.resize(N); occ1.to_u8(dbg.occ1.data(), W, 255); dbg.occ2.resize(N); occ2.to_u8(dbg.occ2.data(), W, 255); dbg.totalArea.resize(N); out.totalArea.to_u8(dbg.totalArea.data(), W, 255); }
    kmLabelLast = out.label3; kmLabelLastAny = maxNum > 0;          // imgLabelLast for the next frame's k-means (DD:1660-1664)
    return SIND_OK;
}

// flow-dependent half: flow masks (DD:1163-1367) and fusion (DD:1553-1636), then the state roll (DD:1660-1664)
int DynaTail::flow_stage(const float* U, const float* V, const DepthStageOut& d, uint8_t* dyna_out, uint8_t* label_out, const float* gridFlowPre, const FlowMasksReady* fm) {
    HIP_TRY(hipSetDevice(cfg.device));
    if (!d.ready) { sind_set_error("DynaTail::flow_stage: the depth stage of this frame has not run"); return SIND_E_STATE; }
    BitImg maskLow, maskHigh; n_frames++;
    { const double t0 = tick_ms(); if (fm) flow_masks_ready(*fm, maskLow, maskHigh); else SIND_TRY(flow_masks(U, V, maskLow, maskHigh, gridFlowPre)); t_stage[0] += tick_ms() - t0; }
    return fuse(maskLow, maskHigh, d, dyna_out, label_out);
}

// fusion (DD:1553-1636) and the state roll (DD:1660-1664)
int DynaTail::fuse(const BitImg& maskLow, const BitImg& maskHigh, const DepthStageOut& d, uint8_t* dyna_out, uint8_t* label_out) {
    double tk = tick_ms();
    #define LAP(i) { const double t_ = tick_ms(); t_stage[i] += t_ - tk; tk = t_; }
    const std::vector<uint8_t>& label3 = d.label3; const int maxNum = d.maxNum; const BitImg& totalArea = d.totalArea;
    double tq = tick_ms();
    #define QLAP(i) { const double t_ = tick_ms(); t_fine[i] += t_ - tq; tq = t_; }
    // fusion (DD:1553-1636)
    BitImg low = highLast; low |= maskLow; low &= totalArea;
    low = low.dilated(EllipseElem(5));
    const BitImg notLow = low.inverted();
    QLAP(25)
    BitImg dyna(W, H);
    std::vector<BitImg> clusters(maxNum + 1); clusters[0].create(W, H);
    if (maxNum > 0) BitImg::split_labels(label3.data(), W, H, W, 1, maxNum, clusters.data() + 1);
    QLAP(26)
    for (int n = 1; n <= maxNum; n++) {
        const BitImg& one = clusters[n]; const int oneCnt = one.count();
        BitImg blocked = one.inverted(), filled(W, H);
        BitImg oneHigh = one; oneHigh &= maskHigh;
        if (oneHigh.count() > 100) {
            std::vector<Contour> cs; find_contours(oneHigh, cs, false);
            for (const Contour& c : cs) {
                const double area = contour_area(c), len = arc_length_closed(c), roundness = (4 * M_PI * area) / (len * len);
                PtI seed{0, 0};
                for (const PtI& p : c) if (low.get(p.x, p.y)) { seed = p; break; }
                if ((area > 100.0 && roundness > 0.2) || area > 2000.0) flood_fill(low.get(seed.x, seed.y) ? low : notLow, blocked, filled, seed);
            }
        }
        if (filled.count() > 0.5 * oneCnt) dyna |= one; else dyna |= filled;
    }
    QLAP(27)
    dyna = dyna.dilated(EllipseElem(9));
    totalArea.to_u8(dyna_out, W, 125); dyna.paint_u8(dyna_out, W, 255);
    std::memcpy(label_out, label3.data(), N);
    // roll the state (DD:1660-1664)
    std::memcpy(dynaLast.data(), dyna_out, N); labelLast = label3; highLast = maskHigh;
    std::memset(lastCnt, 0, sizeof(lastCnt)); std::memset(lastDyn, 0, sizeof(lastDyn));       // per-label pixel / dynamic-pixel counts for the next frame's sample weights
    for (int n = 1; n <= maxNum && n < 256; n++) { lastCnt[n] = clusters[n].count(); lastDyn[n] = BitImg::and_count(clusters[n], dyna); }
    if (hash_state) {
        // imgDynaLast = 255 on `dyna`, 125 on totalArea - dyna, else 0: hashed as those two bit images (canonical: equal byte images give equal words)
        StateHash hs;
        for (size_t i = 0; i < dyna.d.size(); i++) { hs.word(dyna.d[i]); hs.word(totalArea.d[i] & ~dyna.d[i]); hs.word(maskHigh.d[i]); }
        hs.bytes(label3.data(), N); hs.bytes(lastCnt, sizeof(lastCnt)); hs.bytes(lastDyn, sizeof(lastDyn)); hs.word(maxNum > 0 ? 1 : 0);
        hs.finish(state_hash);
    }
    QLAP(28)
    #undef QLAP
    LAP(5)
    #undef LAP
    return SIND_OK;
}

}  // namespace sind
