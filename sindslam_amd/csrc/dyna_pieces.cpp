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
    all.resize(C);                 // (more than 254: the caller reports the capacity error from the count, as on the host path)
    for (int i = 0; i < std::min(C, PIECE_SLOTS); i++) {
        const PieceRecDev& r = h_pieceRecs.p[i]; SegPiece& p = all[i];
        p.cluster = r.cluster; p.clen = r.clen; p.start = PtI{r.sx, r.sy}; p.sum2 = ((long long)r.sum2_hi << 32) | (long long)r.sum2_lo; p.box = Rect{r.x0, r.y0, r.x1, r.y1};
        p.area = (float)r.area; p.cz = r.cz; p.hasLianjie = r.has_conn != 0;
    }
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
        std::vector<SegPiece> all(nc);
        for (int i = 0; i < nc; i++) {
            const PieceRecDev& r = rh[(size_t)b * PIECE_SLOTS + i]; SegPiece& p = all[i];
            p.cluster = r.cluster; p.clen = r.clen; p.start = PtI{r.sx, r.sy}; p.sum2 = ((long long)r.sum2_hi << 32) | (long long)r.sum2_lo; p.box = Rect{r.x0, r.y0, r.x1, r.y1};
            p.area = (float)r.area; p.cz = r.cz; p.hasLianjie = r.has_conn != 0;
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
