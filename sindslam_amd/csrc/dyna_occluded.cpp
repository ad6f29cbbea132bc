// DynaDetect engine, CalOccluded (DD:429-642): the one statement of its GPU front (OccFront), OccBatch for a chunk of frames, and the tail's host halves
// around the PEAC region grow.
#include <cstring>
#include "dyna.hpp"

namespace sind {

// ---- GPU half of CalOccluded (and the 8-bit normalised depth of the RAG statistics) for a chunk of frames in seven launches: the stage has no
// state, so the pipeline runs it for all frames of a step at the step's start instead of seven launches + a stream wait per frame (DD:429-482, 765-768)
int OccFront::init(const DynaConfig& c, int cap_, bool block_stats) {
    cfg = c; cap = cap_; const size_t n = (size_t)c.W * c.H;
    SIND_TRY(filt.alloc(n * cap)); SIND_TRY(edge.alloc(n * cap)); SIND_TRY(edgeTmp.alloc(n * cap)); SIND_TRY(total.alloc(n * cap));
    SIND_TRY(umax.alloc((size_t)2 * cap)); if (block_stats) SIND_TRY(blocks.alloc((size_t)(c.W / 16) * (c.H / 16) * cap));
    return SIND_OK;
}
int OccFront::enqueue_edge(hipStream_t s, const uint16_t* depth_dev, int B, uint8_t* depthN_dev) const {
    if (B < 1 || B > cap) { sind_set_error("OccFront: %d frames (capacity %d)", B, cap); return SIND_E_ARG; }
    const int W = cfg.W, H = cfg.H, N = W * H;
    // the depth-only input of the RAG statistics goes first so that it is finished by the time its consumer waits on the stream
    if (depthN_dev) { SIND_TRY(launch_max_u16(s, depth_dev, N, umax.p + cap, B, 1)); SIND_TRY(launch_depth_norm(s, depth_dev, umax.p + cap, depthN_dev, N, B, 1)); }
    SIND_TRY(launch_median5(s, depth_dev, filt.p, W, H, B));
    SIND_TRY(launch_max_u16(s, filt.p, N, umax.p, B, 1));
    SIND_TRY(launch_grad_edge(s, filt.p, umax.p, edge.p, total.p, W, H, cfg.depthScale, B, 1));
    return SIND_OK;
}
int OccFront::enqueue_open(hipStream_t s, const uint16_t* depth_dev, int B) const {
    if (B < 1 || B > cap) { sind_set_error("OccFront: %d frames (capacity %d)", B, cap); return SIND_E_ARG; }
    const int W = cfg.W, H = cfg.H;
    SIND_TRY(launch_morph(s, edge.p, edgeTmp.p, W, H, 4, false, B));       // MORPH_OPEN, element4 = erode then dilate
    SIND_TRY(launch_morph(s, edgeTmp.p, edge.p, W, H, 4, true, B));
    if (blocks.p) SIND_TRY(launch_peac_block_stats(s, depth_dev, W, H, 16, 16, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.depthScale, blocks.p, B));
    return SIND_OK;
}
int OccBatch::run(hipStream_t s, const uint16_t* depth_dev, int B, uint8_t* depthN_dev, uint8_t* edge_h, uint8_t* total_h, PeacBlockStats* blocks_h) {
    const size_t N = (size_t)front.cfg.W * front.cfg.H, nb = (size_t)(front.cfg.W / 16) * (front.cfg.H / 16);
    SIND_TRY(front.enqueue(s, depth_dev, B, depthN_dev));
    HIP_TRY(hipMemcpyAsync(edge_h, front.edge.p, N * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(total_h, front.total.p, N * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(blocks_h, front.blocks.p, nb * B * sizeof(PeacBlockStats), hipMemcpyDeviceToHost, s));
    return SIND_OK;
}

// ---- DD:429-642: depth-gradient edges (GPU), end points, PEAC plane contours, plane-edge filtering (host).  Two host halves around the PEAC region grow, which runs
// on the GPU (peac_kernels.hip): first half = GPU stencils (unless the batch produced them), packing, end points, PEAC graph clustering and the grow's input block;
// second half = PEAC's last merge + plane contours, contour filter, closing.  grow_block == nullptr: the half grows on the host right away (no GPU grow wanted).
int DynaTail::cal_occluded_p1(const uint16_t* depth_host, const uint16_t* depth_dev, OccCtx& c, const OccGpuOut* pre, uint8_t* grow_block, int depth_index, uint8_t* depthN_dev) {
    double tf = tick_ms();
    #define FLAP(i) { const double t_ = tick_ms(); t_fine[i] += t_ - tf; tf = t_; }
    const uint8_t* edge_h = h_ab.p; const uint8_t* total_h = h_ab.p + N; const PeacBlockStats* blocks_h = h_blocks.data();
    if (pre) { edge_h = pre->edge; total_h = pre->total; blocks_h = pre->blocks; }      // the GPU half ran for all frames of the step at once (OccBatch)
    else {
    SIND_TRY(occ.enqueue(stream, depth_dev, 1, depthN_dev));
    PinnedBuf<PeacBlockStats>& blocks = h_blocks;
    HIP_TRY(hipMemcpyAsync(h_ab.p, occ.edge.p, N, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync((h_ab.p + N), occ.total.p, N, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(blocks.data(), occ.blocks.p, blocks.n * sizeof(PeacBlockStats), hipMemcpyDeviceToHost, stream));
    HIP_TRY(sind_stream_wait(stream));
    }
    FLAP(0)
    c.occ = BitImg::from_u8(edge_h, W, H, W);
    c.totalArea = BitImg::from_u8(total_h, W, H, W);
    if (keep_debug) dbg.gradEdge.assign(edge_h, edge_h + N);
    FLAP(1)
    // end points: edge pixels with at most 4 of the 12 radius-2 ring pixels set (DD:498-532), greedy NMS radius 6 in scan order
    static const int ring[12][2] = {{0,-2},{1,-2},{2,-1},{2,0},{2,1},{1,2},{0,2},{-1,2},{-2,1},{-2,0},{-2,-1},{-1,-2}};
    const BitImg& occ = c.occ;
    std::vector<PtI>& endPoints = c.endPoints; endPoints.clear();
    for (int row = 3; row < H - 3; ++row) {                                     // (edge pixels are sparse: walk the set bits of the row's words, in column order)
        const uint64_t* r = occ.row(row);
        for (int k = 0; k < occ.wpr; k++) for (uint64_t bits = r[k]; bits; bits &= bits - 1) {
            const int col = (k << 6) + __builtin_ctzll(bits);
            if (col < 3 || col >= W - 3) continue;
            int s = 0; for (int i = 0; i < 12; i++) s += occ.get(col + ring[i][0], row + ring[i][1]);
            if (s <= 4) endPoints.push_back({col, row});
        }
    }
    { std::vector<PtI> sel; for (const PtI& e : endPoints) { bool ov = false; for (const PtI& q : sel) { const int dx = e.x - q.x, dy = e.y - q.y; if ((float)dx * dx + dy * dy < 6.0f * 6.0f) { ov = true; break; } } if (!ov) sel.push_back(e); } endPoints.swap(sel); }
    FLAP(2)
    // PEAC (DD:558-593), first part: graph clustering, planes, seeds of the region grow
    PeacInput pin{blocks_h, depth_host, W, H, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.depthScale};
    c.fit.reset(new PeacFitter(pin)); c.fit->part1();
    c.grown_on_host = false;
    if (grow_block) peac_grow_pack(*c.fit, depth_index, grow_block);
    if (!grow_block || !c.fit->gpu_ok) { c.fit->grow_host(c.m8, c.m16, c.pairs); c.grown_on_host = true; }      // beyond the kernel's capacities (or no GPU grow asked for)
    FLAP(3)
    #undef FLAP
    return SIND_OK;
}
int DynaTail::cal_occluded_p2(OccCtx& c, const int8_t* member8, const uint8_t* pair_seen, const int* grow_status, BitImg& occ1, BitImg& occ2) {
    double tf = tick_ms();
    #define FLAP(i) { const double t_ = tick_ms(); t_fine[i] += t_ - tf; tf = t_; }
    BitImg planeC;
    if (!c.fit) { sind_set_error("CalOccluded, second half: the frame has no first half (its PEAC fitter is missing)"); return SIND_E_STATE; }
    if (!c.grown_on_host && !(grow_status && grow_status[0] == PG_OK && member8 && pair_seen)) {
        // the kernel reported a capacity overflow for this frame (status 1..3): the host statement of the same FIFO takes over
        c.fit->grow_host(c.m8, c.m16, c.pairs); c.grown_on_host = true; n_grow_fallback++;
    }
    if (c.grown_on_host) c.fit->part2(c.m8.empty() ? nullptr : c.m8.data(), c.m16.empty() ? nullptr : c.m16.data(), c.pairs.data(), planeC);
    else c.fit->part2(member8, nullptr, pair_seen, planeC);
    c.fit.reset(); c.m8.clear(); c.m16.clear();
    FLAP(3)
    const BitImg& occ = c.occ;
    BitImg edgeByPlane = planeC; edgeByPlane.andnot(occ);                       // DD:599
    std::vector<Contour> contours; find_contours(edgeByPlane, contours, true);
    BitImg acc(W, H);
    const EllipseElem e10(10), e7(7), e3(3);
    for (const Contour& k : contours) {
        if (k.size() < 25) continue;
        BitImg one(W, H); draw_thick2(one, k);
        const Rect bb = contour_bbox(k);
        // "an end point lies in the 10 x 10 dilation of the contour" is asked of the contour itself (the element's window around the end point): the dilation and the
        // erosion are only made for the contours that pass (most do not: the stage was 0.6 ms of a 640 x 480 frame's host time, 1.7 ms at 1280 x 720)
        bool isEnd = false;
        for (const PtI& e : c.endPoints) if (e.y >= bb.y0 - 1 - e10.n && e.y <= bb.y1 + 1 + e10.n && e.x >= bb.x0 - 1 - e10.n && e.x <= bb.x1 + 1 + e10.n && one.dilation_hits(e10, e.x, e.y)) { isEnd = true; break; }
        if (isEnd) { one = one.dilated(e10, bb.y0 - 1, bb.y1 + 1); acc |= one.eroded_rows(e7, bb.y0 - 7, bb.y1 + 7); }
    }
    FLAP(4)
    occ2 = acc;
    BitImg u = occ; u |= acc; occ1 = u.closed(e3);
    FLAP(5)
    #undef FLAP
    if (keep_debug) { dbg.planeContours.resize(N); planeC.to_u8(dbg.planeContours.data(), W, 255); }
    return SIND_OK;
}
// one frame on this tail's own stream: both halves with a one-frame launch of the grow kernel in between
int DynaTail::cal_occluded(const uint16_t* depth_host, const uint16_t* depth_dev, BitImg& totalArea, BitImg& occ1, BitImg& occ2, const OccGpuOut* pre, uint8_t* depthN_dev) {
    // sizes the grow kernel does not take (PeacGrowBatch::supports) are grown on the host in the first half, like before the kernel existed
    const bool gpu_grow = PeacGrowBatch::supports(W, H);
    if (gpu_grow && !own_grow) {
        std::unique_ptr<OwnGrow> g(new OwnGrow());             // assigned only when every piece exists: a failed init must not leave a half-built workspace behind
        SIND_TRY(g->batch.init(W, H, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.depthScale, 1));
        SIND_TRY(g->in_h.alloc(PG_IN_STRIDE)); SIND_TRY(g->member_h.alloc(N)); SIND_TRY(g->pair_h.alloc((size_t)PEAC_GROW_MAX_PLANES * PEAC_GROW_MAX_PLANES)); SIND_TRY(g->status_h.alloc(4));
        own_grow = std::move(g);
    }
    OccCtx c;
    SIND_TRY(cal_occluded_p1(depth_host, depth_dev, c, pre, gpu_grow ? own_grow->in_h.p : nullptr, 0, depthN_dev));
    if (!c.grown_on_host) {
        const double t0 = tick_ms();
        SIND_TRY(own_grow->batch.run(stream, own_grow->in_h.p, depth_dev, 1, own_grow->member_h.p, own_grow->pair_h.p, own_grow->status_h.p));
        HIP_TRY(sind_stream_wait(stream));
        t_fine[33] += tick_ms() - t0;
    }
    SIND_TRY(cal_occluded_p2(c, gpu_grow ? own_grow->member_h.p : nullptr, gpu_grow ? own_grow->pair_h.p : nullptr, gpu_grow ? own_grow->status_h.p : nullptr, occ1, occ2));
    totalArea = c.totalArea;
    return SIND_OK;
}

int DynaTail::compute_occluded(const uint16_t* depth_host, const uint16_t* depth_dev, OccResult& out, const OccGpuOut* pre) {
    HIP_TRY(hipSetDevice(cfg.device));
    // the depth-only input of the RAG statistics rides ahead of the edge chain when this tail makes the chain itself (no `pre`)
    SIND_TRY(cal_occluded(depth_host, depth_dev, out.totalArea, out.occ1, out.occ2, pre, out.depthN_dev));
    return finish_occluded(out, pre);
}
// batched pipeline: first half of a frame (the grow of its chunk is launched by whoever finishes the chunk's last first half) ...
int DynaTail::compute_occluded_p1(const uint16_t* depth_host, const uint16_t* depth_dev, OccCtx& c, const OccGpuOut* pre, uint8_t* grow_block, int depth_index) {
    HIP_TRY(hipSetDevice(cfg.device));
    return cal_occluded_p1(depth_host, depth_dev, c, pre, grow_block, depth_index);
}
// ... and the second half once the chunk's grow results are on the host
int DynaTail::compute_occluded_p2(OccCtx& c, const int8_t* member8, const uint8_t* pair_seen, const int* grow_status, OccResult& out, const OccGpuOut* pre) {
    HIP_TRY(hipSetDevice(cfg.device));
    SIND_TRY(cal_occluded_p2(c, member8, pair_seen, grow_status, out.occ1, out.occ2));
    out.totalArea = c.totalArea;
    return finish_occluded(out, pre);
}
int DynaTail::finish_occluded(OccResult& out, const OccGpuOut* pre) {
    if (out.occ2_dev && pre && pre->occ2_stage && pre->occ2_event) {      // batched path: page-locked staging of the frame's own, consumers wait on the event, not this thread
        out.occ2.to_u8(pre->occ2_stage, W, 255); HIP_TRY(hipMemcpyAsync(out.occ2_dev, pre->occ2_stage, N, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(pre->occ2_event, stream)); out.occ2_event = pre->occ2_event;
    } else if (out.occ2_dev) { out.occ2.to_u8(h_ab.p + N, W, 255); HIP_TRY(hipMemcpyAsync(out.occ2_dev, h_ab.p + N, N, hipMemcpyHostToDevice, stream)); HIP_TRY(sind_stream_wait(stream)); out.occ2_event = nullptr; }
    out.ready = true; return SIND_OK;
}

}  // namespace sind
