// Host stage: piece extraction of SegAndMergeV2 (reference DynaDetect.cc:664-729) on bit images -- every depth cluster minus the occlusion edges is opened, its external
// borders are followed, every border that is long and large enough is filled, grown back into the cluster (the piece), and the part of its thick outline that lies on
// the edge clusters is traced once more for the piece's connection area ("lianjie").  The pieces come out in discovery order: cluster, then raster order of the
// contour's start pixel.  The score, the sort and pieceOf stay with the caller (DynaTail::seg_pieces); sindh_seg_pieces (host_capi.cpp) is the test twin.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>
#include "bitimg.hpp"
#include "contours.hpp"

namespace sind {

// a piece of SegAndMerge (DD:668-760) and its record: the cluster it was cut from, its contour (start pixel, length, twice the signed-area sum as an integer -- every
// term of cv::contourArea's FP64 sum is an integer far below 2^53, so the int64 sum is the same number and area > 80 is |sum2| > 160 -- and bounding box)
struct SegPiece { BitImg img, lianjie; bool hasLianjie = false; float area = 0, score = -10, cz = 0;
                  int cluster = 0, clen = 0, disc = 0; PtI start{0, 0};      // disc: discovery index (set by seg_pieces_rank: it survives the sort)
                  long long sum2 = 0; Rect box{0, 0, -1, -1}; };

inline long long contour_sum2(const Contour& c) {
    if (c.empty()) return 0;
    long long a = 0; PtI prev = c.back();
    for (const PtI& p : c) { a += (long long)prev.x * p.y - (long long)prev.y * p.x; prev = p; }
    return a < 0 ? -a : a;
}

// first raw depth d with (float)d / depthScale >= 6 (65536: none): the comparison is monotonic in d, so "too far" is decided on the raw value
inline int z_invalid_from(float depthScale) {
    int z = 65536;
    for (int d = 65535; d >= 0; d--) { if ((float)(uint16_t)d / depthScale >= (float)(uint16_t)6) z = d; else break; }
    return z;
}
// the score and the order the reference paints the pieces in (DD:731-745).  std::sort is not stable: the result depends on the order the pieces come in
inline void seg_pieces_rank(std::vector<SegPiece>& all) {
    for (size_t i = 0; i < all.size(); i++) all[i].disc = (int)i;
    for (SegPiece& p : all) p.score = (float)(p.area * 0.0003f - p.cz);
    std::sort(all.begin(), all.end(), [](const SegPiece& a, const SegPiece& b) { return a.score > b.score; });
}

// what the device stage (pieces_dev.hpp) knows of a piece, in discovery order (cluster, then raster order of the contour's start pixel); PIECE_SLOTS of them per frame
#define PIECE_SLOTS 255
struct PieceRecDev { int cluster, contour, sx, sy, clen, x0, y0, x1, y1; unsigned sum2_lo; int sum2_hi; int area, band, has_conn; float cz; int pad; };
// the first min(C, PIECE_SLOTS) records as the host's pieces (fields only: the planes stay where the device made them); `all` takes C entries
inline void seg_pieces_from_records(const PieceRecDev* recs, int C, std::vector<SegPiece>& all) {
    all.clear(); all.resize((size_t)std::max(C, 0));
    for (int i = 0; i < std::min(C, PIECE_SLOTS); i++) {
        const PieceRecDev& r = recs[i]; SegPiece& p = all[i];
        p.cluster = r.cluster; p.clen = r.clen; p.start = PtI{r.sx, r.sy}; p.sum2 = (long long)(((unsigned long long)(unsigned)r.sum2_hi << 32) | (unsigned long long)r.sum2_lo); p.box = Rect{r.x0, r.y0, r.x1, r.y1};
        p.area = (float)r.area; p.cz = r.cz; p.hasLianjie = r.has_conn != 0;
    }
}
// The host step between the two device steps of a batched frame (PieceBatch, dyna.hpp), stated once: the records of a frame -> its pieces in RANK order (seg_pieces_rank
// on the discovery sequence: the host function's order, ties included) and the order table the commit kernels read: order[r] = slot (discovery index) of the piece of
// rank r, has_conn[r] = it has a connection area; both take PIECE_SLOTS ints.  Returns C (0: no pieces, nothing ranked), or -1 when C is above 254 (the 8-bit label
// range of the reference: `all` is cleared and the caller reports the count) or negative.
inline int seg_pieces_order(const PieceRecDev* recs, int C, std::vector<SegPiece>& all, int* order, int* has_conn) {
    if (C < 0 || C > 254) { all.clear(); return -1; }
    seg_pieces_from_records(recs, C, all);
    if (C == 0) return 0;
    seg_pieces_rank(all);
    for (int r = 0; r < C; r++) { order[r] = all[r].disc; has_conn[r] = all[r].hasLianjie ? 1 : 0; }
    return C;
}

// The test entries' view of a frame's pieces (sindh_seg_pieces, sind_debug_seg_pieces): the first min(C, cap) pieces in DISCOVERY order as recs [cap][12] ints = cluster,
// start x, start y, contour length, twice the contour area (low, high word), hasLianjie, box x0 y0 x1 y1, rank after the sort (-1 when C is 0 or above 254: nothing is
// ranked then and piece_of is left alone); vals [cap][2] = area, cz; piece / connection planes [cap][h * wpr]; piece_of [h * w] as DynaTail::seg_pieces paints it.
// Ranks `all` on the way.  Returns C.
inline int seg_pieces_export(std::vector<SegPiece>& all, int w, int h, int cap, int* recs, float* vals, uint64_t* piece_planes, uint64_t* conn_planes, uint8_t* piece_of) {
    const size_t pw = (size_t)h * ((w + 63) >> 6);
    const int C = (int)all.size(), n = std::min(C, cap);
    for (int i = 0; i < n; i++) {
        const SegPiece& p = all[i]; int* r = recs + 12 * (size_t)i;
        r[0] = p.cluster; r[1] = p.start.x; r[2] = p.start.y; r[3] = p.clen; r[4] = (int)(uint32_t)(p.sum2 & 0xffffffffll); r[5] = (int)(p.sum2 >> 32); r[6] = p.hasLianjie ? 1 : 0;
        r[7] = p.box.x0; r[8] = p.box.y0; r[9] = p.box.x1; r[10] = p.box.y1; r[11] = -1;
        vals[2 * i] = p.area; vals[2 * i + 1] = p.cz;
        std::memcpy(piece_planes + (size_t)i * pw, p.img.d.data(), pw * 8);
        if (p.hasLianjie) std::memcpy(conn_planes + (size_t)i * pw, p.lianjie.d.data(), pw * 8); else std::memset(conn_planes + (size_t)i * pw, 0, pw * 8);
    }
    if (C == 0 || C > 254) return C;
    seg_pieces_rank(all);
    if (piece_of) std::memset(piece_of, C + 1, (size_t)w * h);
    for (int i = 0; i < C; i++) { const int disc = all[i].disc; if (disc < n) recs[12 * (size_t)disc + 11] = i; if (piece_of) all[i].img.paint_u8(piece_of, w, (uint8_t)i); }
    return C;
}

// planes[0, nCl): the clusters, nearest first; labelForSegEdge: already dilated; depth: H x W u16; a raw depth of 0 or >= zInvalidFrom does not count for cz.
// threads > 1: the clusters go to a few helper threads (same result, same order).  t_fine (optional): the caller's fine-grained stage timers (slots 12 .. 16).
inline void seg_pieces_host(const BitImg* planes, int nCl, const BitImg& occ1, const BitImg& labelForSegEdge, const uint16_t* depth_host, int zInvalidFrom, float invDepthScale,
                            int threads, double* t_fine, std::vector<SegPiece>& all) {
    typedef SegPiece Piece;
    all.clear();
    if (nCl < 1) return;
    const int W = occ1.w, H = occ1.h;
    auto now_ms = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const EllipseElem e4(4), e9(9), e10(10);
    const BitImg occDil = occ1.dilated(e10);
    const float depth_weight = 1.5f;
    // pieces of one depth cluster (DD:668-760); the clusters are independent, the result keeps the cluster order
    auto pieces_of = [&](int i, std::vector<Piece>& out, bool timed) {
        const BitImg& orig = planes[i];
        timed = timed && t_fine;
        double tq = now_ms();
        #define QLAP(i) { if (timed) { const double t_ = now_ms(); t_fine[i] += t_ - tq; tq = t_; } }
        BitImg each = orig; each.andnot(occ1);
        { const Rect eb = each.bbox(); if (eb.empty()) return; each = each.opened_rows(e4, eb.y0, eb.y1); }
        QLAP(12)
        std::vector<Contour> contours; find_contours(each, contours, true);
        QLAP(13)
        for (const Contour& c : contours) {
            if (!(c.size() > 50 && contour_area(c) > 80)) continue;
            tq = now_ms();
            const Rect bb = contour_bbox(c);
            Piece p; p.img.create(W, H); draw_filled(p.img, c);
            p.cluster = i; p.clen = (int)c.size(); p.start = c[0]; p.sum2 = contour_sum2(c); p.box = bb;
            p.img = p.img.dilated(e9, bb.y0, bb.y1); p.img.and_rows(orig, bb.y0 - 4, bb.y1 + 4);       // the 9x9 element reaches 4 rows up and down
            p.area = (float)p.img.count_rows(bb.y0 - 4, bb.y1 + 4);
            QLAP(14)
            BitImg t1(W, H); draw_thick2(t1, c); t1.andnot_rows(occDil, bb.y0 - 1, bb.y1 + 1); t1.and_rows(labelForSegEdge, bb.y0 - 1, bb.y1 + 1);
            if (t1.count_rows(bb.y0 - 1, bb.y1 + 1) > 20) {
                std::vector<Contour> c2; const Rect r2{std::max(bb.x0 - 2, 0), std::max(bb.y0 - 2, 0), std::min(bb.x1 + 2, W - 1), std::min(bb.y1 + 2, H - 1)};
                find_contours(t1, c2, true, &r2);
                std::vector<const Contour*> kept; for (const Contour& q : c2) if (q.size() >= 30) kept.push_back(&q);
                if (!kept.empty()) { p.lianjie.create(W, H); draw_filled(p.lianjie, kept); p.hasLianjie = true; }
            }
            QLAP(15)
            // myCluster::calCenterPoint (DD:256-293): float sums in row-major order; only z is used afterwards
            { float f3 = 0.f; const Rect ib = p.img.bbox();
              for (int y = ib.y0; y <= ib.y1; y++) { const uint64_t* r = p.img.row(y);
                for (int k = 0; k < p.img.wpr; k++) { uint64_t m = r[k]; while (m) { const int x = (k << 6) + __builtin_ctzll(m); m &= m - 1;
                    const uint16_t d = depth_host[(size_t)y * W + x];
                    // (float)d / depthScale >= 6 is monotonic in d: compared against the first raw value that satisfies it (zInvalidFrom)
                    float pzv = 0.f; if (!((int)d >= zInvalidFrom || d == 0)) { const float depth2 = (float)d * invDepthScale; pzv = (float)(depth2 * depth_weight); }
                    f3 += pzv; } } }
              p.cz = f3 / p.area; }
            QLAP(16)
            out.push_back(std::move(p));
        }
        #undef QLAP
    };
    if (threads > 1 && nCl > 1) {        // a stream alone on the GPU (in-order sequence mode) leaves host cores idle: the clusters go to a few helper threads
        std::vector<std::vector<Piece>> per(nCl); std::atomic<int> next{0}; std::vector<std::thread> team;
        auto work = [&] { for (int i; (i = next.fetch_add(1)) < nCl;) pieces_of(i, per[i], false); };
        for (int t = 1; t < std::min(threads, nCl); t++) team.emplace_back(work);
        work();
        for (auto& t : team) t.join();
        for (auto& v : per) for (Piece& q : v) all.push_back(std::move(q));
    } else for (int i = 0; i < nCl; i++) pieces_of(i, all, true);
}

}  // namespace sind
