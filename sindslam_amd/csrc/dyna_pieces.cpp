// Host driver of the device side of SegAndMerge's piece extraction (depth_pieces.hip, pieces_dev.hpp) and its parity entry.
#include <cstring>
#include "../../include/sind_hip.h"
#include "dyna.hpp"

namespace sind {

int PieceTracer::init(int W_, int H_, int cap_, int cap_contours_, int cap_points_, bool own_planes) {
    if (W_ < 1 || H_ < 1 || W_ > 8192 || H_ > 8192 || cap_ < 1 || cap_ > 65535 || cap_contours_ < 1 || cap_points_ < 1) {
        sind_set_error("PieceTracer: %d planes of %d x %d, capacities %d / %d", cap_, W_, H_, cap_contours_, cap_points_); return SIND_E_ARG; }
    W = W_; H = H_; cap = cap_; cap_contours = cap_contours_; cap_points = cap_points_; pw = (size_t)H * ((W + 63) / 64);
    if (own_planes) SIND_TRY(planes.alloc((size_t)cap * pw));
    SIND_TRY(hdr.alloc((size_t)cap * cap_contours)); SIND_TRY(chain.alloc((size_t)cap * cap_points)); SIND_TRY(count.alloc(cap));
    if (piece_cell_words(W, H) * 4 > PIECE_LDS_BYTES) SIND_TRY(scratch.alloc((size_t)cap * piece_cell_words(W, H)));
    return SIND_OK;
}

int PieceStage::init(int W_, int H_, int cap_) {
    if (W_ < 1 || H_ < 1 || W_ > 8192 || H_ > 8192 || cap_ < 1 || cap_ > 64) { sind_set_error("PieceStage: %d frames of %d x %d (1..64 frames)", cap_, W_, H_); return SIND_E_ARG; }
    W = W_; H = H_; cap = cap_; wpr = (W + 63) / 64; pw = (size_t)H * wpr; N = (size_t)W * H;
    const size_t kp = (size_t)cap * PIECE_KMAX * pw, sp = (size_t)cap * PIECE_SLOTS * pw;
    SIND_TRY(in_planes.alloc(kp)); SIND_TRY(tmp.alloc(kp)); SIND_TRY(each.alloc(kp));
    SIND_TRY(occ1.alloc(cap * pw)); SIND_TRY(label_edge.alloc(cap * pw)); SIND_TRY(occ_dil.alloc(cap * pw)); SIND_TRY(depth.alloc(cap * N));
    SIND_TRY(pa.alloc(sp)); SIND_TRY(pb.alloc(sp)); SIND_TRY(pc.alloc(sp)); SIND_TRY(pd.alloc(sp));
    SIND_TRY(recs.alloc((size_t)cap * PIECE_SLOTS)); SIND_TRY(frames.alloc(cap)); SIND_TRY(area.alloc((size_t)cap * PIECE_SLOTS)); SIND_TRY(band.alloc((size_t)cap * PIECE_SLOTS)); SIND_TRY(nplanes_d.alloc(cap));
    SIND_TRY(l1.init(W, H, cap * PIECE_KMAX, PIECE_CONTOUR_CAP, PIECE_CHAIN_CAP, false));
    SIND_TRY(l2.init(W, H, cap * PIECE_SLOTS, PIECE_CONTOUR_CAP2, PIECE_CHAIN_CAP2, false));
    return SIND_OK;
}

// the tail's switch: this frame's pieces from the device stage, in discovery order, as records (the planes stay on the device: seg_pieces_commit).
// *done = false: a plane exceeded a capacity of the stage and the caller runs the host function (counted as fallen back).  A frame with no cluster to cut, more clusters
// than the stage has planes for, or no device depth is left to the host function too and counted as neither.
int DynaTail::seg_pieces_device(const std::vector<BitImg>& allLabels, const BitImg& occ1, const BitImg& labelForSegEdge, std::vector<SegPiece>& all, bool* done) {
    *done = false; all.clear();
    const int nCl = std::max(0, (int)allLabels.size() - 1);
    if (nCl < 1 || nCl > PIECE_KMAX || !segDepthDev) return SIND_OK;
    if (!pieceStage) {
        std::unique_ptr<PieceStage> st(new PieceStage()); SIND_TRY(st->init(W, H, 1));
        SIND_TRY(h_pieceIn.alloc((size_t)(PIECE_KMAX + 2) * st->pw)); SIND_TRY(h_pieceRecs.alloc(PIECE_SLOTS)); SIND_TRY(h_pieceHdr.alloc(1)); SIND_TRY(h_pieceNp.alloc(1));
        SIND_TRY(pieceOf_d.alloc(N)); SIND_TRY(h_pieceOf.alloc(N)); SIND_TRY(pieceOrder_d.alloc(2 * PIECE_SLOTS)); SIND_TRY(h_pieceOrder.alloc(2 * PIECE_SLOTS));
        pieceStage.swap(st);
    }
    PieceStage& st = *pieceStage; const size_t pw = st.pw;
    for (int i = 0; i < nCl; i++) std::memcpy(h_pieceIn.p + (size_t)i * pw, allLabels[i].d.data(), pw * 8);
    std::memcpy(h_pieceIn.p + (size_t)PIECE_KMAX * pw, occ1.d.data(), pw * 8); std::memcpy(h_pieceIn.p + (size_t)(PIECE_KMAX + 1) * pw, labelForSegEdge.d.data(), pw * 8);
    h_pieceNp.p[0] = nCl;
    HIP_TRY(hipMemcpyAsync(st.in_planes.p, h_pieceIn.p, (size_t)nCl * pw * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(st.occ1.p, h_pieceIn.p + (size_t)PIECE_KMAX * pw, pw * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(st.label_edge.p, h_pieceIn.p + (size_t)(PIECE_KMAX + 1) * pw, pw * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(st.nplanes_d.p, h_pieceNp.p, sizeof(int), hipMemcpyHostToDevice, stream));
    SIND_TRY(st.enqueue(stream, 1, segDepthDev, (size_t)N, zInvalidFrom, invDepthScale));
    HIP_TRY(hipMemcpyAsync(h_pieceHdr.p, st.frames.p, sizeof(PieceFrameHdr), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_pieceRecs.p, st.recs.p, PIECE_SLOTS * sizeof(PieceRecDev), hipMemcpyDeviceToHost, stream));
    HIP_TRY(sind_stream_wait(stream));
    const int C = h_pieceHdr.p[0].pieces;
    if (h_pieceHdr.p[0].status != 0 || C < 0) { n_pieces_fallback++; return SIND_OK; }
    *done = true; n_pieces_device++;
    seg_pieces_from_records(h_pieceRecs.p, C, all);                 // (more than 254: the caller reports the capacity error from the count, as on the host path)
    return SIND_OK;
}
// segAll is ranked (disc = the piece's slot in the stage): the order goes up and k_piece_commit writes the planes into planes_d and pieceOf into pieceOf_d.  No wait
int DynaTail::seg_pieces_commit() {
    const int C = (int)segAll.size(); const size_t pw = pieceStage->pw;
    for (int r = 0; r < C; r++) { h_pieceOrder.p[r] = segAll[r].disc; h_pieceOrder.p[PIECE_SLOTS + r] = segAll[r].hasLianjie ? 1 : 0; }
    SIND_TRY(planes_d.alloc((size_t)3 * C * pw));
    HIP_TRY(hipMemcpyAsync(pieceOrder_d.p, h_pieceOrder.p, 2 * PIECE_SLOTS * sizeof(int), hipMemcpyHostToDevice, stream));
    return launch_piece_commit(stream, *pieceStage, 0, C, pieceOrder_d.p, pieceOrder_d.p + PIECE_SLOTS, planes_d.p, pieceOf_d.p);
}
int DynaTail::debug_seg_pieces(const unsigned long long* planes, int k, const unsigned long long* occ1w, const unsigned long long* edgew, const uint16_t* depth_host, const uint16_t* depth_dev,
                               std::vector<SegPiece>& out, std::vector<uint8_t>& piece_of) {
    const size_t pw = (size_t)H * (W / 64);
    auto img = [&](const unsigned long long* q) { BitImg b(W, H); std::memcpy(b.d.data(), q, pw * 8); return b; };
    std::vector<BitImg> labels(k + 1); for (int i = 0; i < k; i++) labels[i] = img(planes + (size_t)i * pw);
    labels[k].create(W, H);                 // (the farthest cluster, which the stage leaves alone)
    segDepthDev = depth_dev; segPre = nullptr;
    SIND_TRY(seg_pieces(labels, img(occ1w), img(edgew), depth_host));
    const int C = (int)segAll.size();
    if (segOnDevice && C > 0) {
        std::vector<unsigned long long> pl((size_t)3 * C * pw); piece_of.resize(N);
        HIP_TRY(hipMemcpyAsync(pl.data(), planes_d.p, pl.size() * 8, hipMemcpyDeviceToHost, stream)); HIP_TRY(hipMemcpyAsync(piece_of.data(), pieceOf_d.p, N, hipMemcpyDeviceToHost, stream));
        HIP_TRY(sind_stream_wait(stream));
        for (int r = 0; r < C; r++) { SegPiece& p = segAll[r]; p.img.create(W, H); std::memcpy(p.img.d.data(), pl.data() + (size_t)r * pw, pw * 8);
            p.lianjie.create(W, H); std::memcpy(p.lianjie.d.data(), pl.data() + ((size_t)2 * C + r) * pw, pw * 8); }
    } else piece_of = segPieceOf;
    out = segAll; segAll.clear(); segOnDevice = false;
    return SIND_OK;
}
void DynaTail::debug_set_piece_inputs(const unsigned long long* planes, int k, const unsigned long long* occ1w, const unsigned long long* edgew, const uint16_t* depth_host,
                                      const uint16_t* depth_dev, const OccResult* pre) {
    const size_t pw = (size_t)H * (W / 64);
    auto img = [&](const unsigned long long* q) { BitImg b(W, H); std::memcpy(b.d.data(), q, pw * 8); return b; };
    segLabels.assign(k + 1, BitImg(W, H)); for (int i = 0; i < k; i++) segLabels[i] = img(planes + (size_t)i * pw);      // (the last one: the farthest cluster, which is not cut)
    segOcc1 = img(occ1w); segEdge = img(edgew); segDepthHost = depth_host; segDepthDev = depth_dev; segPre = pre; segAll.clear(); segOnDevice = false;
}

// ---- the piece stage of one frame of every stream of a k-means group, in chunks (see dyna.hpp)
int PieceBatch::init(const DynaConfig& c, int max_frames, hipStream_t s) {
    cfg = c; W = c.W; H = c.H; cap = max_frames; stream = s; pw = (size_t)H * (W / 64); N = (size_t)W * H;
    if (W % 64 != 0 || max_frames < 1) { sind_set_error("PieceBatch: width must be a multiple of 64 (got %d), %d frames", W, max_frames); return SIND_E_ARG; }
    set_chunk(chunk_n);
    return SIND_OK;
}
PieceBatch::~PieceBatch() { for (hipEvent_t e : done) if (e) (void)hipEventDestroy(e); }
int PieceBatch::begin_round() {
    HIP_TRY(hipSetDevice(cfg.device));
    if (!ready || st.cap < chunk_n) {
        SIND_TRY(st.init(W, H, chunk_n));      // (an allocation that fails is the round's failure, with hipMalloc's text)
        SIND_TRY(dtab_d.alloc(chunk_n)); SIND_TRY(crec_d.alloc(chunk_n)); SIND_TRY(crec_h.alloc((size_t)cap)); SIND_TRY(tab_d.alloc((size_t)chunk_n * 2 * PIECE_SLOTS));
        SIND_TRY(pof_d.alloc((size_t)cap * N)); SIND_TRY(pof_h.alloc((size_t)cap * N));
        SIND_TRY(planes_h.alloc((size_t)cap * PIECE_KMAX * pw)); SIND_TRY(occ1_h.alloc((size_t)cap * pw)); SIND_TRY(edge_h.alloc((size_t)cap * pw)); SIND_TRY(np_h.alloc(cap)); SIND_TRY(dtab_h.alloc(cap));
        SIND_TRY(hdr_h.alloc(cap)); SIND_TRY(recs_h.alloc((size_t)cap * PIECE_SLOTS)); SIND_TRY(tab_h.alloc((size_t)cap * 2 * PIECE_SLOTS));
        if (done.empty()) { done.assign(cap, nullptr); for (hipEvent_t& e : done) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
        ready = true;
    }
    std::lock_guard<std::mutex> lk(m);
    n_slots = 0;
    return SIND_OK;
}
int PieceBatch::take_slot() { std::lock_guard<std::mutex> lk(m); return ready && n_slots < cap ? n_slots++ : -1; }
void PieceBatch::pack(int slot, const BitImg* labels, int nCl, const BitImg& occ1, const BitImg& label_edge, const uint16_t* depth_dev) {
    nCl = std::max(0, std::min(nCl, PIECE_KMAX));
    for (int i = 0; i < nCl; i++) std::memcpy(planes_h.p + ((size_t)slot * PIECE_KMAX + i) * pw, labels[i].d.data(), pw * 8);
    std::memcpy(occ1_h.p + (size_t)slot * pw, occ1.d.data(), pw * 8); std::memcpy(edge_h.p + (size_t)slot * pw, label_edge.d.data(), pw * 8);
    np_h.p[slot] = nCl; dtab_h.p[slot] = depth_dev;
}
int PieceBatch::enqueue(int chunk, int z_invalid_from, float inv_depth_scale) {
    HIP_TRY(hipSetDevice(cfg.device));
    int first, n; { std::lock_guard<std::mutex> lk(m); first = chunk_first(chunk); n = chunk_count(chunk); }
    if (chunk < 0 || n < 1 || n > st.cap) { sind_set_error("PieceBatch::enqueue: chunk %d holds %d frames (capacity %d)", chunk, n, st.cap); return SIND_E_ARG; }
    for (int b = first; b < first + n; b++) if (!dtab_h.p[b]) { sind_set_error("PieceBatch::enqueue: slot %d has no depth plane", b); return SIND_E_STATE; }
    // (planes a frame does not have keep what an earlier frame left in the slab: the kernels stop at the frame's plane count)
    HIP_TRY(hipMemcpyAsync(st.in_planes.p, planes_h.p + (size_t)first * PIECE_KMAX * pw, (size_t)n * PIECE_KMAX * pw * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(st.occ1.p, occ1_h.p + (size_t)first * pw, (size_t)n * pw * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(st.label_edge.p, edge_h.p + (size_t)first * pw, (size_t)n * pw * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(st.nplanes_d.p, np_h.p + first, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(dtab_d.p, dtab_h.p + first, (size_t)n * sizeof(const uint16_t*), hipMemcpyHostToDevice, stream));
    SIND_TRY(st.enqueue(stream, n, nullptr, 0, z_invalid_from, inv_depth_scale, dtab_d.p));
    HIP_TRY(hipMemcpyAsync(hdr_h.p + first, st.frames.p, (size_t)n * sizeof(PieceFrameHdr), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(recs_h.p + (size_t)first * PIECE_SLOTS, st.recs.p, (size_t)n * PIECE_SLOTS * sizeof(PieceRecDev), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(done[chunk], stream));
    return SIND_OK;
}
int PieceBatch::wait(int chunk) {
    if (chunk < 0 || chunk >= (int)done.size()) { sind_set_error("PieceBatch::wait: chunk %d", chunk); return SIND_E_ARG; }
    HIP_TRY(sind_event_wait(done[chunk]));
    return SIND_OK;
}
int PieceBatch::commit(int chunk, int n, const int* slots, const int* C, const size_t* plane_off, unsigned long long* slab, size_t slab_words) {
    if (n < 1) return SIND_OK;
    HIP_TRY(hipSetDevice(cfg.device));
    const int first = chunk_first(chunk);
    if (n > st.cap) { sind_set_error("PieceBatch::commit: %d frames, capacity %d", n, st.cap); return SIND_E_ARG; }
    for (int i = 0; i < n; i++) {
        const int b = slots[i] - first;
        if (b < 0 || b >= chunk_n || (i > 0 && slots[i] <= slots[i - 1])) { sind_set_error("PieceBatch::commit: slot %d is not of chunk %d", slots[i], chunk); return SIND_E_ARG; }
        crec_h.p[first + i] = PieceCommitRec{(unsigned long long)plane_off[i], (unsigned long long)((size_t)slots[i] * N), b, C[i], b * 2 * PIECE_SLOTS, 0};
    }
    const int lo = slots[0], hi = slots[n - 1];
    HIP_TRY(hipMemcpyAsync(tab_d.p + (size_t)(lo - first) * 2 * PIECE_SLOTS, tab_h.p + (size_t)lo * 2 * PIECE_SLOTS, (size_t)(hi - lo + 1) * 2 * PIECE_SLOTS * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(crec_d.p, crec_h.p + first, (size_t)n * sizeof(PieceCommitRec), hipMemcpyHostToDevice, stream));
    SIND_TRY(launch_piece_commit_frames(stream, st, crec_d.p, crec_h.p + first, n, tab_d.p, (size_t)chunk_n * 2 * PIECE_SLOTS, slab, slab_words, pof_d.p, (size_t)cap * N));
    // pieceOf of the frames between the first and the last committed one in one copy (a fallen-back frame in between rides along unused)
    HIP_TRY(hipMemcpyAsync(pof_h.p + (size_t)lo * N, pof_d.p + (size_t)lo * N, (size_t)(hi - lo + 1) * N, hipMemcpyDeviceToHost, stream));
    return SIND_OK;
}

int piece_chunk_flush(PieceBatch& pb, RagBatch& rb, int chunk, PieceChunkFrame* fr) {
    const int first = pb.chunk_first(chunk), n = pb.chunk_count(chunk);
    if (n < 1 || n > 64) { sind_set_error("piece_chunk_flush: chunk %d holds %d frames", chunk, n); return SIND_E_ARG; }
    if (pb.stream != rb.stream) { sind_set_error("piece_chunk_flush: the piece and the RAG batch must share a stream (the commit is ordered in front of the RAG launches by it)"); return SIND_E_STATE; }
    int C[64], rag_slots[64], cslots[64], cC[64], m = 0, nc = 0, idx[64]; uint8_t dev[64]; unsigned long long *pieces[64], *conn[64]; size_t coff[64];
    int run_first = -1, run_n = 0;
    {
        std::lock_guard<std::mutex> lk(pb.flush_mutex());
        SIND_TRY(pb.enqueue(chunk, fr[0].half->piece_z_invalid_from(), fr[0].half->piece_inv_depth_scale()));
        SIND_TRY(pb.wait(chunk));
        // the host step: records -> ranked pieces and the order table; a frame beyond a capacity of the stage runs the host function here
        for (int i = 0; i < n; i++) {
            PieceChunkFrame& f = fr[i]; const PieceFrameHdr& h = pb.header(first + i);
            f.rc = SIND_OK; f.err.clear(); f.rag_slot = -1; f.own = false; f.on_device = false; f.fell_back = h.status != 0 || h.pieces < 0;
            int* tab = pb.order_table(first + i);
            f.rc = f.fell_back ? f.half->seg_pieces_batched(nullptr, 0, nullptr, nullptr) : f.half->seg_pieces_batched(pb.records(first + i), h.pieces, tab, tab + PIECE_SLOTS);
            if (f.rc != SIND_OK) { f.err = sind_last_error(); continue; }
            if (f.half->rag_pieces() < 1) continue;
            f.on_device = !f.fell_back;
            idx[m] = i; C[m] = f.half->rag_pieces(); dev[m] = f.on_device ? 1 : 0; m++;
        }
        // the run: consecutive slots of the RAG batch, the planes of the frames that stayed on the device written there by the commit kernels
        if (m > 0) run_first = rb.reserve_run(m, C, dev, rag_slots, pieces, conn);
        for (int k = 0; k < m; k++) {
            PieceChunkFrame& f = fr[idx[k]];
            if (rag_slots[k] < 0) {      // no room in the slabs: the per-frame stage, from host planes
                f.own = true;
                if (f.on_device) { f.on_device = false; f.fell_back = true; f.rc = f.half->seg_pieces_batched(nullptr, 0, nullptr, nullptr); if (f.rc != SIND_OK) f.err = sind_last_error(); }
                continue;
            }
            f.rag_slot = rag_slots[k]; run_n++;
            const OccResult* pre = f.half->rag_pre(); rb.set_inputs(f.rag_slot, pre->occ2_dev, pre->depthN_dev, pre->occ2_event);
            if (f.on_device) { cslots[nc] = first + idx[k]; cC[nc] = C[k]; coff[nc] = rb.plane_off(f.rag_slot); nc++; }
            else f.half->rag_pack(pieces[k], conn[k]);
        }
        SIND_TRY(pb.commit(chunk, nc, cslots, cC, coff, rb.slab_dev(), rb.slab_words()));
        if (run_n > 0) SIND_TRY(rb.enqueue_run(run_first, run_n, chunk));
    }
    if (run_n > 0) SIND_TRY(rb.wait(chunk));      // (the counters, and pieceOf in front of them on the stream)
    return SIND_OK;
}

}  // namespace sind

extern "C" {

// parity-test access to the whole device stage (PieceStage at capacity n) and the host function: see include/sind_hip.h
int sind_debug_seg_pieces(const unsigned long long* planes, int k, const unsigned long long* occ1, const unsigned long long* label_edge, const uint16_t* depth, int n, int width, int height,
                          float depth_scale, int device, int cap, int* info_gpu, int* recs_gpu, float* vals_gpu, unsigned long long* pieces_gpu, unsigned long long* conn_gpu, uint8_t* piece_of_gpu,
                          int* info_host, int* recs_host, float* vals_host, unsigned long long* pieces_host, unsigned long long* conn_host, uint8_t* piece_of_host) {
    if (!planes || !occ1 || !label_edge || !depth || !info_gpu || !recs_gpu || !vals_gpu || !pieces_gpu || !conn_gpu || !piece_of_gpu || !info_host || !recs_host || !vals_host || !pieces_host ||
        !conn_host || !piece_of_host || k < 1 || k > PIECE_KMAX || n < 1 || n > 64 || width < 1 || height < 1 || width > 8192 || height > 8192 || cap < 1 || cap > PIECE_SLOTS || !(depth_scale > 0)) {
        sind_set_error("sind_debug_seg_pieces: bad arguments (1..64 frames of 1..%d planes, 1..%d records)", PIECE_KMAX, PIECE_SLOTS); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    using namespace sind;
    if (n == 1) {
        // ---- one frame: a tail of its own with the switch on -- its capacity-1 stage on its stream, the fallback, the ranking, k_piece_commit.  info = C, fell back, the counters
        if (width % 64 != 0 || height % 8 != 0) { sind_set_error("sind_debug_seg_pieces: one frame runs through a tail (width a multiple of 64, height of 8)"); return SIND_E_ARG; }
        const size_t pw1 = (size_t)height * (width / 64), N1 = (size_t)width * height;
        DynaConfig cfg; cfg.W = width; cfg.H = height; cfg.depthScale = depth_scale; cfg.device = device;
        hipStream_t ts = nullptr; HIP_TRY(hipStreamCreateWithFlags(&ts, hipStreamNonBlocking));
        int rc = SIND_OK;
        {
            DynaTail tail; DevBuf<uint16_t> dd; std::vector<SegPiece> got; std::vector<uint8_t> po;
            rc = tail.init(cfg, ts);
            if (rc == SIND_OK) rc = dd.alloc(N1);
            if (rc == SIND_OK && hipMemcpyAsync(dd.p, depth, N1 * 2, hipMemcpyHostToDevice, ts) != hipSuccess) { sind_set_error("sind_debug_seg_pieces: depth upload failed"); rc = SIND_E_HIP; }
            if (rc == SIND_OK && sind_stream_wait(ts) != hipSuccess) { sind_set_error("sind_debug_seg_pieces: stream wait failed"); rc = SIND_E_HIP; }
            tail.device_pieces = true;
            if (rc == SIND_OK) rc = tail.debug_seg_pieces(planes, k, occ1, label_edge, depth, dd.p, got, po);
            if (rc == SIND_OK) {
                // back into discovery order for the export, which ranks again (same comparator on the same sequence: the same order)
                const int C = (int)got.size(); std::vector<SegPiece> disc(C);
                for (int r = 0; r < C; r++) disc[got[r].disc] = got[r];
                info_gpu[0] = seg_pieces_export(disc, width, height, cap, recs_gpu, vals_gpu, reinterpret_cast<uint64_t*>(pieces_gpu), reinterpret_cast<uint64_t*>(conn_gpu), nullptr);
                if (C > 0) std::memcpy(piece_of_gpu, po.data(), N1);
                for (int r = 0; r < C; r++) if (disc[r].disc != got[r].disc) { sind_set_error("sind_debug_seg_pieces: the export ranked the pieces differently from the tail"); rc = SIND_E_STATE; }
                info_gpu[1] = tail.n_pieces_fallback > 0 ? 1 : 0; info_gpu[2] = (int)tail.n_pieces_device; info_gpu[3] = (int)tail.n_pieces_fallback;
            } else if (rc == SIND_E_CAPACITY) {         // more than 254 pieces: the tail's own error, text kept in sind_last_error; the count is in its debug block
                info_gpu[0] = tail.dbg.nClusters; info_gpu[1] = tail.n_pieces_fallback > 0 ? 1 : 0; info_gpu[2] = (int)tail.n_pieces_device; info_gpu[3] = (int)tail.n_pieces_fallback; rc = SIND_OK;
            }
        }
        (void)hipStreamDestroy(ts);
        if (rc != SIND_OK) return rc;
        std::vector<BitImg> cl(k); for (int i = 0; i < k; i++) { cl[i].create(width, height); std::memcpy(cl[i].d.data(), planes + (size_t)i * pw1, pw1 * 8); }
        BitImg o1(width, height), le(width, height); std::memcpy(o1.d.data(), occ1, pw1 * 8); std::memcpy(le.d.data(), label_edge, pw1 * 8);
        std::vector<SegPiece> hall;
        seg_pieces_host(cl.data(), k, o1, le, depth, z_invalid_from(depth_scale), 1.0f / depth_scale, 1, nullptr, hall);
        info_host[0] = seg_pieces_export(hall, width, height, cap, recs_host, vals_host, reinterpret_cast<uint64_t*>(pieces_host), reinterpret_cast<uint64_t*>(conn_host), piece_of_host);
        info_host[1] = info_host[2] = info_host[3] = 0;
        return SIND_OK;
    }
    PieceStage st; SIND_TRY(st.init(width, height, n));
    const size_t pw = st.pw, N = st.N; const int zinv = z_invalid_from(depth_scale); const float inv = 1.0f / depth_scale;
    std::vector<int> np(n, k);
    for (int b = 0; b < n; b++) HIP_TRY(hipMemcpy(st.in_planes.p + (size_t)b * PIECE_KMAX * pw, planes + (size_t)b * k * pw, (size_t)k * pw * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st.occ1.p, occ1, (size_t)n * pw * 8, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(st.label_edge.p, label_edge, (size_t)n * pw * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st.depth.p, depth, (size_t)n * N * 2, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(st.nplanes_d.p, np.data(), n * sizeof(int), hipMemcpyHostToDevice));
    SIND_TRY(st.enqueue(nullptr, n, nullptr, 0, zinv, inv));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<PieceFrameHdr> fh(n); std::vector<PieceRecDev> rh((size_t)n * PIECE_SLOTS);
    HIP_TRY(hipMemcpy(fh.data(), st.frames.p, n * sizeof(PieceFrameHdr), hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(rh.data(), st.recs.p, rh.size() * sizeof(PieceRecDev), hipMemcpyDeviceToHost));
    auto img = [&](const unsigned long long* p) { BitImg b(width, height); std::memcpy(b.d.data(), p, pw * 8); return b; };
    for (int b = 0; b < n; b++) {
        // ---- the device's pieces as the host's type, then the same export (ranking, pieceOf) for both sides
        const int C = fh[b].pieces, nc = std::min(std::max(C, 0), PIECE_SLOTS);
        std::vector<SegPiece> all; seg_pieces_from_records(rh.data() + (size_t)b * PIECE_SLOTS, nc, all);
        for (int i = 0; i < nc; i++) {
            SegPiece& p = all[i];
            p.img.create(width, height); HIP_TRY(hipMemcpy(p.img.d.data(), st.pb.p + ((size_t)b * PIECE_SLOTS + i) * pw, pw * 8, hipMemcpyDeviceToHost));
            if (p.hasLianjie) { p.lianjie.create(width, height); HIP_TRY(hipMemcpy(p.lianjie.d.data(), st.pa.p + ((size_t)b * PIECE_SLOTS + i) * pw, pw * 8, hipMemcpyDeviceToHost)); }
        }
        if (C > PIECE_SLOTS) all.resize(C);                 // (more than 254 pieces: only the count matters, nothing is ranked)
        info_gpu[4 * b] = seg_pieces_export(all, width, height, std::min(cap, nc), recs_gpu + (size_t)b * cap * 12, vals_gpu + (size_t)b * cap * 2, reinterpret_cast<uint64_t*>(pieces_gpu + (size_t)b * cap * pw),
                                            reinterpret_cast<uint64_t*>(conn_gpu + (size_t)b * cap * pw), piece_of_gpu + (size_t)b * N);
        info_gpu[4 * b + 1] = fh[b].status; info_gpu[4 * b + 2] = info_gpu[4 * b + 3] = 0;
        std::vector<BitImg> cl(k); for (int i = 0; i < k; i++) cl[i] = img(planes + ((size_t)b * k + i) * pw);
        std::vector<SegPiece> hall;
        seg_pieces_host(cl.data(), k, img(occ1 + (size_t)b * pw), img(label_edge + (size_t)b * pw), depth + (size_t)b * N, zinv, inv, 1, nullptr, hall);
        info_host[4 * b] = seg_pieces_export(hall, width, height, cap, recs_host + (size_t)b * cap * 12, vals_host + (size_t)b * cap * 2, reinterpret_cast<uint64_t*>(pieces_host + (size_t)b * cap * pw),
                                             reinterpret_cast<uint64_t*>(conn_host + (size_t)b * cap * pw), piece_of_host + (size_t)b * N);
        info_host[4 * b + 1] = info_host[4 * b + 2] = info_host[4 * b + 3] = 0;
    }
    return SIND_OK;
}

// parity-test access to the round's batched piece stage (PieceBatch, piece_chunk_flush, the commit kernels, the RAG launches on the device slab) against the host
// function packed from the host: see include/sind_hip.h
int sind_debug_pieces_batch(const unsigned long long* planes, int k, const unsigned long long* occ1, const unsigned long long* label_edge, const uint16_t* depth, const uint8_t* occ2,
                            const uint8_t* depth_n, int n, int width, int height, float depth_scale, int device, int chunk, int cap, int rag_cap,
                            int* info_gpu, int* recs_gpu, float* vals_gpu, unsigned long long* pieces_gpu, unsigned long long* conn_gpu, uint8_t* piece_of_gpu, int* rag_gpu,
                            int* info_host, int* recs_host, float* vals_host, unsigned long long* pieces_host, unsigned long long* conn_host, uint8_t* piece_of_host, int* rag_host) {
    if (!planes || !occ1 || !label_edge || !depth || !occ2 || !depth_n || !info_gpu || !recs_gpu || !vals_gpu || !pieces_gpu || !conn_gpu || !piece_of_gpu || !rag_gpu || !info_host || !recs_host ||
        !vals_host || !pieces_host || !conn_host || !piece_of_host || !rag_host || k < 1 || k > PIECE_KMAX || n < 1 || n > 64 || chunk < 1 || chunk > 64 || width < 64 || width % 64 != 0 || height < 8 ||
        height % 8 != 0 || width > 8192 || height > 8192 || cap < 1 || cap > PIECE_SLOTS || rag_cap < 1 || !(depth_scale > 0)) {
        sind_set_error("sind_debug_pieces_batch: bad arguments (1..64 frames of 1..%d planes, chunks of 1..64, width a multiple of 64, height of 8, 1..%d records)", PIECE_KMAX, PIECE_SLOTS); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    using namespace sind;
    const size_t pw = (size_t)height * (width / 64), N = (size_t)width * height;
    DynaConfig cfg; cfg.W = width; cfg.H = height; cfg.depthScale = depth_scale; cfg.device = device;
    hipStream_t ts = nullptr; HIP_TRY(hipStreamCreateWithFlags(&ts, hipStreamNonBlocking));
    auto run = [&]() -> int {
        // the frames' depth planes at growing distances: no one stride reaches them, the stage reads them through its table
        std::vector<size_t> doff(n); size_t dtotal = 0; for (int b = 0; b < n; b++) { dtotal += (size_t)1024 * b; doff[b] = dtotal; dtotal += N; }
        DevBuf<uint16_t> dd; DevBuf<uint8_t> o2, dn; SIND_TRY(dd.alloc(dtotal)); SIND_TRY(o2.alloc((size_t)n * N)); SIND_TRY(dn.alloc((size_t)n * N));
        for (int b = 0; b < n; b++) HIP_TRY(hipMemcpyAsync(dd.p + doff[b], depth + (size_t)b * N, N * 2, hipMemcpyHostToDevice, ts));
        HIP_TRY(hipMemcpyAsync(o2.p, occ2, (size_t)n * N, hipMemcpyHostToDevice, ts)); HIP_TRY(hipMemcpyAsync(dn.p, depth_n, (size_t)n * N, hipMemcpyHostToDevice, ts));
        HIP_TRY(sind_stream_wait(ts));
        std::vector<std::unique_ptr<DynaTail>> tails(n); std::vector<OccResult> pre(n);
        for (int b = 0; b < n; b++) { tails[b].reset(new DynaTail()); SIND_TRY(tails[b]->init(cfg, ts)); pre[b].ready = true; pre[b].occ2_dev = o2.p + (size_t)b * N; pre[b].depthN_dev = dn.p + (size_t)b * N; }
        for (int side = 0; side < 2; side++) {       // 0: the host function, packed from the host (today's path); 1: the batched device stage
            int* info = side ? info_gpu : info_host; int* recs = side ? recs_gpu : recs_host; float* vals = side ? vals_gpu : vals_host; int* rag_out = side ? rag_gpu : rag_host;
            uint64_t* pl_out = reinterpret_cast<uint64_t*>(side ? pieces_gpu : pieces_host); uint64_t* cn_out = reinterpret_cast<uint64_t*>(side ? conn_gpu : conn_host); uint8_t* po_out = side ? piece_of_gpu : piece_of_host;
            RagBatch rb; PieceBatch pb; std::vector<PieceChunkFrame> fr(n);
            SIND_TRY(rb.init(cfg, n, ts)); rb.set_limits(chunk, 128); SIND_TRY(rb.begin_round());
            for (int b = 0; b < n; b++) { tails[b]->debug_set_piece_inputs(planes + (size_t)b * k * pw, k, occ1 + (size_t)b * pw, label_edge + (size_t)b * pw, depth + (size_t)b * N, dd.p + doff[b], &pre[b]); fr[b] = PieceChunkFrame(); fr[b].half = tails[b].get(); }
            if (side) {
                SIND_TRY(pb.init(cfg, n, ts)); pb.set_chunk(chunk); SIND_TRY(pb.begin_round());
                for (int b = 0; b < n; b++) {
                    DynaTail& t = *tails[b];
                    if (!t.piece_batchable() || pb.take_slot() != b) { sind_set_error("sind_debug_pieces_batch: frame %d did not get its slot", b); return SIND_E_STATE; }
                    pb.pack(b, t.piece_labels().data(), k, t.piece_occ1(), t.piece_edge(), t.piece_depth_dev());
                }
                for (int c = 0; c * pb.chunk_frames() < n; c++) SIND_TRY(piece_chunk_flush(pb, rb, c, fr.data() + pb.chunk_first(c)));
            } else {
                for (int b = 0; b < n; b++) {
                    PieceChunkFrame& f = fr[b]; DynaTail& t = *tails[b];
                    f.rc = t.seg_pieces_batched(nullptr, 0, nullptr, nullptr);
                    if (f.rc != SIND_OK) { f.err = sind_last_error(); continue; }
                    if (t.rag_pieces() < 1) continue;
                    unsigned long long *pc = nullptr, *cn = nullptr;
                    if (rb.reserve(t.rag_pieces(), &f.rag_slot, &pc, &cn)) { t.rag_pack(pc, cn); rb.set_inputs(f.rag_slot, pre[b].occ2_dev, pre[b].depthN_dev, nullptr); } else { f.rag_slot = -1; f.own = true; }
                }
                for (int c = 0; c * rb.chunk_frames() < rb.slots(); c++) { SIND_TRY(rb.enqueue(c)); SIND_TRY(rb.wait(c)); }
            }
            std::string cap_err;
            for (int b = 0; b < n; b++) {
                PieceChunkFrame& f = fr[b]; DynaTail& t = *tails[b]; int* inf = info + 4 * b;
                if (f.rc != SIND_OK) {          // more than 254 pieces: the count and the code; the text stays in sind_last_error
                    if (f.rc != SIND_E_CAPACITY) { sind_set_error("%s", f.err.c_str()); return f.rc; }
                    inf[0] = t.dbg.nClusters; inf[1] = f.rc; inf[2] = f.fell_back ? 1 : 0; inf[3] = 0; cap_err = f.err; continue;
                }
                std::vector<SegPiece> got = t.debug_pieces(); const int C = (int)got.size();
                inf[0] = C; inf[1] = 0; inf[2] = f.fell_back ? 1 : 0; inf[3] = f.on_device ? 1 : 0;
                if (C == 0) continue;
                if (rag_result_ints(C) > (size_t)rag_cap) { sind_set_error("sind_debug_pieces_batch: frame %d has %d pieces, its RAG block does not fit %d ints", b, C, rag_cap); return SIND_E_CAPACITY; }
                std::vector<unsigned long long> raw;
                if (f.on_device) {          // the planes as the commit kernels left them in the RAG batch's device slab: [0, C) pieces, [C, 2C) connection areas, rank order
                    raw.resize((size_t)2 * C * pw);
                    HIP_TRY(hipMemcpyAsync(raw.data(), rb.slab_dev() + rb.plane_off(f.rag_slot), raw.size() * 8, hipMemcpyDeviceToHost, ts)); HIP_TRY(sind_stream_wait(ts));
                    for (int r = 0; r < C; r++) { SegPiece& p = got[r]; p.img.create(width, height); std::memcpy(p.img.d.data(), raw.data() + (size_t)r * pw, pw * 8);
                        p.lianjie.create(width, height); std::memcpy(p.lianjie.d.data(), raw.data() + ((size_t)C + r) * pw, pw * 8); }
                }
                std::vector<SegPiece> disc(C); for (int r = 0; r < C; r++) disc[got[r].disc] = got[r];
                int* rc12 = recs + (size_t)b * cap * 12; uint64_t* cn_b = cn_out + (size_t)b * cap * pw;
                seg_pieces_export(disc, width, height, cap, rc12, vals + (size_t)b * cap * 2, pl_out + (size_t)b * cap * pw, cn_b, nullptr);
                for (int r = 0; r < C; r++) if (disc[r].disc != got[r].disc) { sind_set_error("sind_debug_pieces_batch: the export ranked the pieces of frame %d differently", b); return SIND_E_STATE; }
                if (f.on_device) for (int i = 0; i < std::min(C, cap); i++) std::memcpy(cn_b + (size_t)i * pw, raw.data() + ((size_t)C + rc12[12 * i + 11]) * pw, pw * 8);      // (what the device wrote, zeros of a missing connection area included)
                std::memcpy(po_out + (size_t)b * N, f.on_device ? pb.piece_of(b) : t.debug_piece_of().data(), N);
                const int* rag = nullptr;
                if (f.rag_slot >= 0) rag = rb.result(f.rag_slot); else SIND_TRY(t.rag_own(&rag));
                std::memcpy(rag_out + (size_t)b * rag_cap, rag, rag_result_ints(C) * sizeof(int));
            }
            if (!cap_err.empty()) sind_set_error("%s", cap_err.c_str());
        }
        return SIND_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(ts); (void)hipStreamDestroy(ts);
    return rc;
}

// parity-test access to k_piece_contours: see include/sind_hip.h
int sind_debug_contours(const unsigned long long* planes, int n, int width, int height, int device, int cap_contours, int cap_points,
                        int* counts_gpu, int* hdr_gpu, int* pts_gpu, int* counts_host, int* hdr_host, int* pts_host) {
    if (!planes || !counts_gpu || !hdr_gpu || !pts_gpu || !counts_host || !hdr_host || !pts_host || n < 1 || n > 4096 || width < 1 || height < 1 || width > 8192 || height > 8192 ||
        cap_contours < 1 || cap_contours > (1 << 20) || cap_points < 1 || cap_points > (1 << 24)) {
        sind_set_error("sind_debug_contours: bad arguments (1..4096 planes of at most 8192 x 8192, capacities >= 1)"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    sind::PieceTracer tr; SIND_TRY(tr.init(width, height, n, cap_contours, cap_points));
    HIP_TRY(hipMemcpy(tr.planes.p, planes, (size_t)n * tr.pw * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(tr.count.p, 0xff, (size_t)n * sizeof(sind::PiecePlaneCount)));      // a plane the launch forgets shows
    SIND_TRY(tr.enqueue(nullptr, n));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<sind::PiecePlaneCount> cnt(n); std::vector<sind::PieceContourHdr> hd((size_t)n * cap_contours); std::vector<unsigned> ch((size_t)n * cap_points);
    HIP_TRY(hipMemcpy(cnt.data(), tr.count.p, cnt.size() * sizeof(cnt[0]), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hd.data(), tr.hdr.p, hd.size() * sizeof(hd[0]), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ch.data(), tr.chain.p, ch.size() * sizeof(ch[0]), hipMemcpyDeviceToHost));
    std::memset(hdr_gpu, 0, (size_t)n * cap_contours * 10 * sizeof(int)); std::memset(pts_gpu, 0, (size_t)n * cap_points * 2 * sizeof(int));
    std::memset(hdr_host, 0, (size_t)n * cap_contours * 10 * sizeof(int)); std::memset(pts_host, 0, (size_t)n * cap_points * 2 * sizeof(int));
    for (int i = 0; i < n; i++) {
        const sind::PiecePlaneCount& c = cnt[i];
        counts_gpu[3 * i] = c.contours; counts_gpu[3 * i + 1] = c.points; counts_gpu[3 * i + 2] = c.status;
        if (c.contours < 0 || c.contours > cap_contours || c.points < 0 || c.points > cap_points) { sind_set_error("sind_debug_contours: plane %d reports %d contours, %d points", i, c.contours, c.points); return SIND_E_STATE; }
        for (int k = 0; k < c.contours; k++) std::memcpy(hdr_gpu + ((size_t)i * cap_contours + k) * 10, &hd[(size_t)i * cap_contours + k], 10 * sizeof(int));
        for (int k = 0; k < c.points; k++) { const unsigned v = ch[(size_t)i * cap_points + k]; int* q = pts_gpu + ((size_t)i * cap_points + k) * 2; q[0] = (int)(v & 0xffffu); q[1] = (int)(v >> 16); }
        // the host function on the same plane: the totals, and what fits the capacities
        sind::BitImg b(width, height); std::memcpy(b.d.data(), planes + (size_t)i * tr.pw, tr.pw * 8);
        std::vector<sind::Contour> cs; sind::find_contours(b, cs, true);
        int np = 0, nc = 0;
        for (const sind::Contour& q : cs) {
            if (nc < cap_contours) {
                const sind::Rect r = sind::contour_bbox(q); const long long s2 = sind::contour_sum2(q);
                const int h10[10] = {q[0].x, q[0].y, (int)q.size(), np, r.x0, r.y0, r.x1, r.y1, (int)(unsigned)(s2 & 0xffffffffll), (int)(s2 >> 32)};
                std::memcpy(hdr_host + ((size_t)i * cap_contours + nc) * 10, h10, sizeof(h10));
            }
            nc++;
            for (const sind::PtI& p : q) { if (np < cap_points) { int* o = pts_host + ((size_t)i * cap_points + np) * 2; o[0] = p.x; o[1] = p.y; } np++; }
        }
        counts_host[3 * i] = nc; counts_host[3 * i + 1] = np; counts_host[3 * i + 2] = nc > cap_contours ? PIECE_ST_CONTOURS : np > cap_points ? PIECE_ST_POINTS : PIECE_ST_OK;
    }
    return SIND_OK;
}

}  // extern "C"
