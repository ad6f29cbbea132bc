// DynaDetect engine, SegAndMergeV2 (DD:653-1018, cal_hist :1685-1739): pieces on the host (host/pieces.hpp; opt-in on the GPU: dyna_pieces.cpp), region-adjacency statistics on the GPU (per frame, or RagBatch for one frame
// of every stream of a k-means group), greedy merge on the host.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <thread>
#include "dyna.hpp"

namespace sind {

// ---- DD:653-1018: split every depth cluster on edges into pieces, region-adjacency statistics on the GPU, greedy merge on the host
// host part up to the pieces in score order and pieceOf; they stay in segAll / segPieceOf (no pieces: segAll is empty and the frame's labels are all 0)
int DynaTail::seg_pieces(const std::vector<BitImg>& allLabels, const BitImg& occ1, const BitImg& labelForSegEdge, const uint16_t* depth_host, bool allow_device) {
    typedef SegPiece Piece;
    std::vector<Piece>& all = segAll; all.clear();
    double tf = tick_ms();
    bool on_device = false;
    if (device_pieces && allow_device) SIND_TRY(seg_pieces_device(allLabels, occ1, labelForSegEdge, all, &on_device));      // (counts the frame as on the device or as fallen back)
    segOnDevice = on_device;
    if (!on_device) seg_pieces_host(allLabels.data(), std::max(0, (int)allLabels.size() - 1), occ1, labelForSegEdge, depth_host, zInvalidFrom, invDepthScale, piece_threads, t_fine, all);      // (host/pieces.hpp)
    t_fine[6] += tick_ms() - tf;
    return seg_pieces_check_and_rank(on_device);
}
static int too_many_pieces(int C) { sind_set_error("seg_and_merge: %d pieces exceed the 8-bit label range of the reference", C); return SIND_E_CAPACITY; }
int DynaTail::seg_pieces_check_and_rank(bool on_device) {
    std::vector<SegPiece>& all = segAll;
    const double tf = tick_ms();
    const int C = (int)all.size();
    dbg.nClusters = C;
    if (C == 0) { segOnDevice = false; return SIND_OK; }
    if (C > 254) { all.clear(); segOnDevice = false; return too_many_pieces(C); }
    seg_pieces_rank(all);
    if (on_device) SIND_TRY(seg_pieces_commit());      // the planes stay on the device, in rank order in the RAG stage's layout; pieceOf is painted there and comes back with the RAG counters
    else {
        segPieceOf.assign(N, (uint8_t)(C + 1));       // index of the piece that owns a pixel (the reference paints the pieces in score order)
        for (int i = 0; i < C; i++) all[i].img.paint_u8(segPieceOf.data(), W, (uint8_t)i);
    }
    t_fine[10] += tick_ms() - tf;
    return SIND_OK;
}
// the second part of process_begin for a frame of a round's PieceBatch: its records, ranked (the planes are committed on the device, pieceOf comes with process_end),
// or -- recs = nullptr: the frame exceeded a capacity of the device stage -- the host function, whatever the tail's own switch says
int DynaTail::seg_pieces_batched(const PieceRecDev* recs, int C, int* order, int* has_conn) {
    segOnDevice = false;
    if (!recs) return seg_pieces(segLabels, segOcc1, segEdge, segDepthHost, false);
    const double tf = tick_ms();
    const int n = seg_pieces_order(recs, C, segAll, order, has_conn);      // (host/pieces.hpp)
    t_fine[10] += tick_ms() - tf;
    dbg.nClusters = C;
    if (n < 0) return too_many_pieces(C);
    return SIND_OK;
}
// the pieces' planes and their connection areas' (zeros for a piece without one), C planes of H * W / 64 words each
void DynaTail::rag_pack(unsigned long long* pieces, unsigned long long* conn) const {
    const int C = (int)segAll.size(); const size_t pw = (size_t)H * (W / 64);
    for (int i = 0; i < C; i++) {
        std::memcpy(pieces + (size_t)i * pw, segAll[i].img.d.data(), pw * 8);
        if (segAll[i].hasLianjie) std::memcpy(conn + (size_t)i * pw, segAll[i].lianjie.d.data(), pw * 8); else std::memset(conn + (size_t)i * pw, 0, pw * 8);
    }
}
int DynaTail::rag_own(const int** rag) { HIP_TRY(hipSetDevice(cfg.device)); const double t0 = tick_ms(); const int r = seg_rag_gpu(rag); t_stage[4] += tick_ms() - t0; return r; }
// ---- the GPU stage for this frame alone (every path that is not batched): upload the 2*C bit planes, dilation, one pass over the frame, the counters back, one wait
int DynaTail::seg_rag_gpu(const int** rag_out) {
    const int C = (int)segAll.size(); const BitImg& occ2 = segOcc2; const OccResult* pre = segPre; const uint16_t* depth_dev = segDepthDev;
    double tf = tick_ms();
    #define FLAP(i) { const double t_ = tick_ms(); t_fine[i] += t_ - tf; tf = t_; }
    const int wpr = W / 64; const size_t pw = (size_t)H * wpr;
    SIND_TRY(h_rag.alloc((size_t)3 * C * C + C + (size_t)C * 256));
    const size_t planes_n = (size_t)3 * C * pw;
    // plane sets: [0, C) pieces, [C, 2C) their 7x7 dilations (formed on the GPU from the first set), [2C, 3C) connection areas
    if (segOnDevice) {         // k_piece_commit wrote the first and the third set already (seg_pieces_commit, which sized planes_d): no pack, no upload
        SIND_TRY(rag_d.alloc((size_t)3 * C * C + C + (size_t)C * 256));
        if (planes_d.n < planes_n) { sind_set_error("seg_rag_gpu: the committed planes are missing"); return SIND_E_STATE; }
    } else {
        SIND_TRY(h_planes.alloc((size_t)3 * C * pw));
        unsigned long long* planes = h_planes.p;
        rag_pack(planes, planes + (size_t)2 * C * pw);
        FLAP(10)
        SIND_TRY(planes_d.alloc(planes_n)); SIND_TRY(rag_d.alloc((size_t)3 * C * C + C + (size_t)C * 256));
        FLAP(11)
        HIP_TRY(hipMemcpyAsync(planes_d.p, planes, (size_t)C * pw * 8, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(planes_d.p + (size_t)2 * C * pw, planes + (size_t)2 * C * pw, (size_t)C * pw * 8, hipMemcpyHostToDevice, stream));
    }
    SIND_TRY(launch_dilate_planes(stream, planes_d.p, planes_d.p + (size_t)C * pw, C, W, H, 7, rag_d.p, (int)((size_t)3 * C * C + C + (size_t)C * 256)));      // also clears the RAG accumulators
    const uint8_t* occ2_use = pre && pre->occ2_dev ? pre->occ2_dev : occ2_d.p;
    if (pre && pre->occ2_dev && pre->occ2_event) HIP_TRY(hipStreamWaitEvent(stream, pre->occ2_event, 0));       // uploaded on the CalOccluded runner's stream without a host wait
    if (!(pre && pre->occ2_dev)) { occ2.to_u8((h_ab.p + N), W, 255); HIP_TRY(hipMemcpyAsync(occ2_d.p, (h_ab.p + N), N, hipMemcpyHostToDevice, stream)); }
    FLAP(7)
    const uint8_t* depthN_use = pre && pre->depthN_dev ? pre->depthN_dev : depthN.p;
    if (!(pre && pre->depthN_dev)) { SIND_TRY(launch_max_u16(stream, depth_dev, N, occ.umax.p + 1)); SIND_TRY(launch_depth_norm(stream, depth_dev, occ.umax.p + 1, depthN.p, N)); }      // (the raw-maximum slot of the one-frame OccFront)
    int* ov_d = rag_d.p; int* ovp_d = ov_d + C * C; int* lj_d = ovp_d + C * C; int* la_d = lj_d + C * C; int* hist_dd = la_d + C;
    SIND_TRY(launch_rag_stats(stream, planes_d.p, C, W, H, wpr, occ2_use, depthN_use, ov_d, ovp_d, lj_d, la_d, hist_dd, true));
    PinnedBuf<int>& rag = h_rag;
    HIP_TRY(hipMemcpyAsync(rag.data(), rag_d.p, ((size_t)3 * C * C + C + (size_t)C * 256) * sizeof(int), hipMemcpyDeviceToHost, stream));
    if (segOnDevice) HIP_TRY(hipMemcpyAsync(h_pieceOf.p, pieceOf_d.p, N, hipMemcpyDeviceToHost, stream));      // pieceOf rides under the same wait
    HIP_TRY(sind_stream_wait(stream));
    if (segOnDevice) segPieceOf.assign(h_pieceOf.p, h_pieceOf.p + N);
    FLAP(8)
    #undef FLAP
    *rag_out = rag.data();
    return SIND_OK;
}
// host part from the counters on: cal_hist, merge matrix, folds, labelNew
void DynaTail::seg_finish(const int* rag, std::vector<uint8_t>& labelNew) {
    const std::vector<SegPiece>& all = segAll; const std::vector<uint8_t>& pieceOf = segPieceOf; const int C = (int)all.size();
    double tf = tick_ms();
    #define FLAP(i) { const double t_ = tick_ms(); t_fine[i] += t_ - tf; tf = t_; }
    const int* ov = rag; const int* ovp = ov + C * C; const int* ljo = ovp + C * C; const int* lja = ljo + C * C; const int* hst = lja + C;
    // cal_hist (DD:1685-1739) from the two masked histograms
    auto cal_hist = [&](int a, int b, double out[3]) {
        float h1[256], h2[256]; double m1 = 0, m2 = 0, mn1 = DBL_MAX, mn2 = DBL_MAX;
        for (int i = 0; i < 256; i++) { h1[i] = (float)hst[a * 256 + i]; h2[i] = (float)hst[b * 256 + i]; m1 = std::max<double>(m1, h1[i]); m2 = std::max<double>(m2, h2[i]); mn1 = std::min<double>(mn1, h1[i]); mn2 = std::min<double>(mn2, h2[i]); }
        const int hist_h = 400;
        auto norm_minmax = [&](float* h, double mn, double mx) { const double scale = (mx - mn) > DBL_EPSILON ? (double)hist_h / (mx - mn) : 0, shift = 0 - mn * scale; for (int i = 0; i < 256; i++) h[i] = h[i] * (float)scale + (float)shift; };
        if (m1 > m2) { norm_minmax(h1, mn1, m1); const float s = (float)(1.0 / (m1 / hist_h)); for (int i = 0; i < 256; i++) h2[i] = h2[i] * s; }
        else         { norm_minmax(h2, mn2, m2); const float s = (float)(1.0 / (m2 / hist_h)); for (int i = 0; i < 256; i++) h1[i] = h1[i] * s; }
        double s1 = 0, s2 = 0, s11 = 0, s12 = 0, s22 = 0, bh = 0, inter = 0;
        for (int j = 0; j < 256; j++) { const double x = h1[j], y = h2[j]; s12 += x * y; s1 += x; s11 += x * x; s2 += y; s22 += y * y; bh += std::sqrt(x * y); inter += std::min(h1[j], h2[j]); }
        const double scale = 1. / 256, num = s12 - s1 * s2 * scale, denom2 = (s11 - s1 * s1 * scale) * (s22 - s2 * s2 * scale);
        out[0] = std::fabs(denom2) > DBL_EPSILON ? num / std::sqrt(denom2) : 1.;
        double ss = s1 * s2; ss = std::fabs(ss) > FLT_EPSILON ? 1. / std::sqrt(ss) : 1.;
        out[1] = 1 - std::sqrt(std::max(1. - bh * ss, 0.));
        out[2] = inter;
    };
    const int M = C + 1, numCluster = KM_K;
    std::vector<float> mTotal((size_t)M * M, 0.f), m2((size_t)M * M, 0.f), m3((size_t)M * M, 0.f), wgt((size_t)M * M, 1.f), rej((size_t)M * M, 1.f);
    const float thredshold = 0.9f; const int smallLabel = (int)std::min(0.7f * C, 15.0f);
    for (int i = 0; i < C; i++) for (int j = i + 1; j < C; j++) {
        float v2 = 0, v3 = 0, lessArea; int lessLabel;
        if (all[i].area < all[j].area) { lessArea = all[i].area; lessLabel = i; } else { lessArea = all[j].area; lessLabel = j; }
        if (lessLabel < 10) wgt[i * M + j] = wgt[j * M + i] = 0.7f;
        else if (lessLabel > smallLabel) wgt[i * M + j] = wgt[j * M + i] = 2.0f;
        const int overlap = ov[i * C + j], overlapPlane = ovp[i * C + j];
        if (overlap > std::min(200.0f, lessArea * 0.4f)) {
            double isMerge[3]; cal_hist(i, j, isMerge);
            v3 = (float)(isMerge[0] + isMerge[1] + isMerge[2] * 0.0005);
            if (overlapPlane > 100 && lessLabel < smallLabel) { rej[i * M + j] = rej[j * M + i] = 0.f; continue; }
            else if (v3 < 0.19f && lessLabel < smallLabel) { rej[i * M + j] = rej[j * M + i] = 0.f; continue; }
            if (all[i].hasLianjie && all[j].hasLianjie) {
                const int o = ljo[i * C + j];
                if (o > 0) { const int a1 = lja[i], a2 = lja[j];
                    if (o > std::min(50, (int)(0.5 * std::min(a1, a2)))) { v2 = (float)o; if ((o > 0.62 * a1) || (o > 0.62 * a2)) v2 = (float)std::max(250, o); } }
            }
            m2[i * M + j] = m2[j * M + i] = v2; m3[i * M + j] = m3[j * M + i] = v3;
        }
    }
    for (size_t k = 0; k < mTotal.size(); k++) mTotal[k] = ((m2[k] * 0.01f + m3[k]) * rej[k]) * wgt[k];
    int countMerged = 0;
    std::vector<std::vector<int>> merge(M); std::vector<int> mergeSit(M, 0);
    auto fold = [&](int dst, int j) {
        std::vector<float> col(M); for (int r = 0; r < M; r++) col[r] = mTotal[r * M + j];
        for (int r = 0; r < M; r++) mTotal[r * M + dst] += col[r];
        for (int c = 0; c < M; c++) mTotal[dst * M + c] += col[c];
        for (int r = 0; r < M; r++) mTotal[r * M + j] = 0.f;
        for (int c = 0; c < M; c++) mTotal[j * M + c] = 0.f;
    };
    for (int i = 0; i < std::min(numCluster - 1 + countMerged, C); i++)
        for (int j = i + 1; j < std::min(numCluster - 1 + countMerged, C); j++) {
            const float sorce = mTotal[j * M + i];
            if (sorce > thredshold) {
                int toMerge = i; const float toMergeValue = mTotal[j * M + i];
                for (int k = 0; k < j; k++) if (mTotal[k * M + j] > toMergeValue) toMerge = k;
                mergeSit[j] = 1; merge[toMerge].push_back(j); fold(toMerge, j); countMerged++;
            }
        }
    for (int i = std::min(numCluster - 1 + countMerged, C); i < C; i++) {
        int mergeCluster = C; float maxScore = 0.2f;
        for (int j = 0; j < i; j++) { const float score = mTotal[j * M + i]; if (score > maxScore) { maxScore = score; mergeCluster = j; } }
        mergeSit[i] = 1; merge[mergeCluster].push_back(i); fold(mergeCluster, i);
    }
    int labelindex = 1; std::vector<uint8_t> lut(256, 0);
    for (int i = 0; i < C; i++) {
        if (mergeSit[i]) continue;
        std::vector<char> sel(M + 1, 0); sel[i] = 1;
        for (int mj : merge[i]) { sel[mj] = 1; for (int mk : merge[mj]) sel[mk] = 1; }
        // the reference paints labels in increasing order, a later group overwrites an earlier one on shared pieces
        for (int q = 0; q <= M; q++) if (sel[q]) lut[q] = (uint8_t)labelindex;
        labelindex++;
    }
    for (int k = 0; k < N; k++) labelNew[k] = lut[pieceOf[k]];
    FLAP(9)
    #undef FLAP
}

// ---- the GPU stage of SegAndMerge for one frame of every stream of a k-means group, in chunks (see dyna.hpp)
int RagBatch::init(const DynaConfig& c, int max_frames, hipStream_t s) {
    cfg = c; W = c.W; H = c.H; cap = max_frames; stream = s; pw = (size_t)H * (W / 64);
    if (W % 64 != 0 || max_frames < 1) { sind_set_error("RagBatch: width must be a multiple of 64 (got %d), %d frames", W, max_frames); return SIND_E_ARG; }
    SIND_TRY(recs_h.alloc(cap)); SIND_TRY(recs_d.alloc(cap));
    occ2_ev.assign(cap, nullptr); done.resize(cap, nullptr); on_dev.assign(cap, 0);
    for (hipEvent_t& e : done) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return SIND_OK;
}
RagBatch::~RagBatch() { for (hipEvent_t e : done) if (e) (void)hipEventDestroy(e); }
int RagBatch::begin_round() {
    HIP_TRY(hipSetDevice(cfg.device));
    // result blocks: 16 K ints per frame hold 40 pieces (3 C^2 + 257 C); a frame that does not fit takes the per-frame stage
    in_cap = (size_t)cap * planes_frame * pw; res_cap = (size_t)cap * 16384;
    SIND_TRY(in_h.alloc(std::max<size_t>(in_cap, 2))); SIND_TRY(in_d.alloc(std::max<size_t>(in_cap, 2))); SIND_TRY(dil_d.alloc(std::max<size_t>(in_cap / 2, 1)));
    SIND_TRY(res_d.alloc(res_cap)); SIND_TRY(res_h.alloc(res_cap));
    std::lock_guard<std::mutex> lk(m);
    n_slots = 0; in_used = 0; res_used = 0;
    return SIND_OK;
}
bool RagBatch::reserve_locked(int C, bool dev, int* slot, unsigned long long** pieces, unsigned long long** conn) {
    if (C < 1 || C > 254) return false;
    const size_t words = (size_t)2 * C * pw, ints = rag_result_ints(C);
    if (n_slots >= cap || in_used + words > in_cap || res_used + ints > res_cap) return false;
    RagRec& R = recs_h.p[n_slots];
    R.plane_off = in_used; R.res_off = res_used; R.C = C; R.pad = 0; R.occ2 = nullptr; R.depthN = nullptr;
    on_dev[n_slots] = dev ? 1 : 0;
    *pieces = in_h.p + in_used; *conn = *pieces + (size_t)C * pw; *slot = n_slots++;
    in_used += words; res_used += ints;
    return true;
}
bool RagBatch::reserve(int C, int* slot, unsigned long long** pieces, unsigned long long** conn) {
    std::lock_guard<std::mutex> lk(m);
    return reserve_locked(C, false, slot, pieces, conn);
}
int RagBatch::reserve_run(int n, const int* C, const uint8_t* on_device, int* slots, unsigned long long** pieces, unsigned long long** conn) {
    std::lock_guard<std::mutex> lk(m);      // (held over the run: its slots and planes are consecutive)
    int first = -1;
    for (int i = 0; i < n; i++) {
        slots[i] = -1;
        if (reserve_locked(C[i], on_device[i] != 0, &slots[i], &pieces[i], &conn[i]) && first < 0) first = slots[i];
    }
    return first;
}
void RagBatch::set_inputs(int slot, const uint8_t* occ2, const uint8_t* depthN, hipEvent_t ev) { recs_h.p[slot].occ2 = occ2; recs_h.p[slot].depthN = depthN; occ2_ev[slot] = ev; }
int RagBatch::enqueue(int chunk) {
    int first, n; { std::lock_guard<std::mutex> lk(m); first = chunk_first(chunk); n = chunk_count(chunk); }
    if (chunk < 0 || n < 1) { sind_set_error("RagBatch::enqueue: chunk %d holds no frame", chunk); return SIND_E_ARG; }
    return enqueue_run(first, n, chunk);
}
int RagBatch::enqueue_run(int first, int n, int ev) {
    HIP_TRY(hipSetDevice(cfg.device));
    { std::lock_guard<std::mutex> lk(m); if (first < 0 || n < 1 || first + n > n_slots || ev < 0 || ev >= cap) { sind_set_error("RagBatch::enqueue_run: slots [%d, %d) of %d, event %d", first, first + n, n_slots, ev); return SIND_E_ARG; } }
    const int chunk = ev;
    const RagRec& A = recs_h.p[first]; const RagRec& Z = recs_h.p[first + n - 1];
    const size_t r0 = A.res_off, r1 = Z.res_off + rag_result_ints(Z.C);
    std::lock_guard<std::mutex> lk(enq);      // (two chunks of a round may be enqueued by two pool threads: one chunk's calls stay together on the stream)
    for (int b = first; b < first + n; b++) if (occ2_ev[b]) HIP_TRY(hipStreamWaitEvent(stream, occ2_ev[b], 0));       // occ2 uploaded on the CalOccluded runner's stream without a host wait
    // the planes of every run of host-packed slots in one copy (all of them, where no slot's planes lie in the device slab already: one copy, as ever)
    for (int b = first; b < first + n;) {
        if (on_dev[b]) { b++; continue; }
        int e = b; while (e + 1 < first + n && !on_dev[e + 1]) e++;
        const size_t w0 = recs_h.p[b].plane_off, w1 = recs_h.p[e].plane_off + (size_t)2 * recs_h.p[e].C * pw;
        HIP_TRY(hipMemcpyAsync(in_d.p + w0, in_h.p + w0, (w1 - w0) * 8, hipMemcpyHostToDevice, stream));
        b = e + 1;
    }
    HIP_TRY(hipMemcpyAsync(recs_d.p + first, recs_h.p + first, (size_t)n * sizeof(RagRec), hipMemcpyHostToDevice, stream));
    SIND_TRY(launch_rag_frames(stream, recs_d.p + first, recs_h.p + first, n, in_d.p, in_cap, dil_d.p, res_d.p, res_cap, W, H));
    HIP_TRY(hipMemcpyAsync(res_h.p + r0, res_d.p + r0, (r1 - r0) * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(done[chunk], stream));
    return SIND_OK;
}
int RagBatch::wait(int chunk) {
    if (chunk < 0 || chunk >= cap) { sind_set_error("RagBatch::wait: chunk %d", chunk); return SIND_E_ARG; }
    HIP_TRY(sind_event_wait(done[chunk]));
    return SIND_OK;
}

}  // namespace sind
