// Device side of SegAndMerge's piece extraction (depth_pieces.hip, driver dyna_pieces.cpp): external borders of bit planes on the GPU, bit for bit what
// find_contours(external_only) of host/contours.hpp returns -- the same borders in the same order (raster order of the start pixel), the same points in the same order.
//
// Capacities (every device loop is bounded by one of them, none by the data alone):
//   cap_contours   contours per plane   (PIECE_CONTOUR_CAP by default)
//   cap_points     chain points per plane, over all its contours (PIECE_CHAIN_CAP by default); one trace walks at most the points that are left
//   the scan visits at most (W + 2)(H + 2) value changes of a plane, and looks for the next one in at most (W + 2)(H + 2) / 1024 + 1 steps
// A plane that exceeds a capacity ends with status PIECE_ST_CONTOURS / PIECE_ST_POINTS; what it wrote up to there is valid and the caller takes the host function.
// The scan's marks are 2-bit cells ((W + 2)(H + 2) / 4 bytes: 77 KB at 640 x 480) in LDS where they fit PIECE_LDS_BYTES, else in a global scratch plane.
#pragma once
#include "common.hpp"
#include "depth.hpp"
#include "host/pieces.hpp"

namespace sind {

#define PIECE_CONTOUR_CAP 1024
#define PIECE_CHAIN_CAP 32768
#define PIECE_LDS_BYTES (144 * 1024)          /* of the CU's 160 KiB */
#define PIECE_ST_OK 0
#define PIECE_ST_CONTOURS 1
#define PIECE_ST_POINTS 2

// one border: start pixel, number of points, where its points begin in the plane's chain, bounding box, and twice its signed-area sum as cv::contourArea forms it
// (sum over the closed chain of x[i-1] y[i] - y[i-1] x[i]; integers, so the int64 sum is the FP64 sum), absolute value, in two words
struct PieceContourHdr { int sx, sy, len, off, x0, y0, x1, y1; unsigned sum2_lo; int sum2_hi; };
struct PiecePlaneCount { int contours, points, status, pad; };

// size in 32-bit words of one plane's mark cells
static inline size_t piece_cell_words(int W, int H) { return ((size_t)(W + 2) * (H + 2) + 15) / 16; }
// planes: [nplanes][H * wpr] words (device); per plane: hdr [cap_contours], chain [cap_points] (x | y << 16), count.  scratch: nplanes * piece_cell_words(W, H) words when the
// cells do not fit the LDS (else unused, may be nullptr).  One wave per plane, one launch whatever the planes hold.
// gate (optional, one int per plane): a plane whose gate is <= gate_min is not followed and reports nothing
int launch_piece_contours(hipStream_t s, const unsigned long long* planes, int nplanes, int W, int H, PieceContourHdr* hdr, unsigned* chain, PiecePlaneCount* count,
                          int cap_contours, int cap_points, unsigned* scratch, const int* gate = nullptr, int gate_min = 0);

// workspaces for up to `cap` planes of W x H, made once: no allocation per call once it is warm
struct PieceTracer {
    int W = 0, H = 0, cap = 0, cap_contours = PIECE_CONTOUR_CAP, cap_points = PIECE_CHAIN_CAP; size_t pw = 0;
    DevBuf<unsigned long long> planes; DevBuf<PieceContourHdr> hdr; DevBuf<unsigned> chain, scratch; DevBuf<PiecePlaneCount> count;
    int init(int W, int H, int cap, int cap_contours = PIECE_CONTOUR_CAP, int cap_points = PIECE_CHAIN_CAP, bool own_planes = true);      // own_planes = false: the caller traces planes of its own
    // launches only: the planes are in `planes` already
    int enqueue(hipStream_t s, int nplanes) { return launch_piece_contours(s, planes.p, nplanes, W, H, hdr.p, chain.p, count.p, cap_contours, cap_points, scratch.p); }
};

// ---- the whole stage, stated once for `cap` frames of up to PIECE_KMAX cluster planes (DD:664-729; the ranking stays on the host) ------------------------------------
// Further capacities: PIECE_SLOTS pieces per frame (a frame with more than 254 is an error of the stage anyway); second level (the band planes): PIECE_CONTOUR_CAP2
// contours and PIECE_CHAIN_CAP2 chain points per piece.  A frame in which a plane exceeds a capacity reports status != 0 and the caller runs the host function for it.
#define PIECE_KMAX 12
#define PIECE_CONTOUR_CAP2 256
#define PIECE_CHAIN_CAP2 16384
// (PIECE_SLOTS and PieceRecDev, what the device knows of a piece, are stated in host/pieces.hpp, where the host step that reads them lives)
struct PieceFrameHdr { int pieces, status, pad0, pad1; };
struct PieceStage {
    int W = 0, H = 0, wpr = 0, cap = 0; size_t pw = 0, N = 0;
    // inputs of frame b: in_planes + (b * PIECE_KMAX + i) * pw, occ1 / label_edge + b * pw, depth + b * N; nplanes[b] (host) cluster planes
    DevBuf<unsigned long long> in_planes, occ1, label_edge, occ_dil, tmp, each, pa, pb, pc, pd; DevBuf<uint16_t> depth;
    DevBuf<PieceRecDev> recs; DevBuf<PieceFrameHdr> frames; DevBuf<int> area, band, nplanes_d;
    PieceTracer l1, l2;
    int init(int W, int H, int cap);
    // launches only (13 of them whatever the frames hold): afterwards recs [b][PIECE_SLOTS] / frames [b] hold the records, pb the piece planes and pa the connection planes
    // of frame b at (b * PIECE_SLOTS + slot) * pw.  nplanes_d must hold the frames' plane counts; depth_dev: nullptr = the stage's own `depth`.
    // depth_tab (device, optional): n pointers, frame b's depth plane is depth_tab[b] -- frames that come from arbitrary streams lie at no one stride; without it frame b
    // lies at depth_dev + b * depth_stride (the table's special case, same bits)
    int enqueue(hipStream_t s, int n, const uint16_t* depth_dev, size_t depth_stride, int z_invalid_from, float inv_depth_scale, const uint16_t* const* depth_tab = nullptr);
};
// k_piece_commit for one frame of a stage (frame b): the host has ranked the C pieces (order_dev[r] = slot of the piece of rank r, has_conn_dev[r] = it has a connection area);
// the planes go in rank order straight into the RAG stage's layout -- pieces into planes_out [0, C), connection planes (zeros where a piece has none) into [2C, 3C) -- and
// piece_of_out [H * W] takes the rank of the piece that owns a pixel (the highest rank wins, as painting in rank order does), C + 1 elsewhere.  Two launches.
int launch_piece_commit(hipStream_t s, const PieceStage& st, int b, int C, const int* order_dev, const int* has_conn_dev, unsigned long long* planes_out, uint8_t* piece_of_out);
// The same for the frames of a chunk at once (PieceBatch, dyna.hpp), straight into the BATCHED RAG stage's slab (RagRec of depth.hpp): frame i of the list is frame
// `b` of the stage and has C ranked pieces; its order table (order[r] = slot of rank r at table + tab_off, has_conn[r] at table + tab_off + PIECE_SLOTS) came up with the
// list.  k_piece_commit_frames writes the pieces into slab [plane_off, + C planes) and the connection planes into the C planes behind them -- the batch's [0, C) / [C, 2C)
// layout, not the per-frame [0, C) / [2C, 3C) -- zeros for a piece without a connection area; k_piece_paint_frames writes pieceOf [H * W] at piece_of + piece_of_off
// (highest rank wins, C + 1 where no piece is).  Two launches whatever the list holds; `host` is the list as the device will see it (bounds are checked on it).
struct PieceCommitRec { unsigned long long plane_off, piece_of_off; int b, C, tab_off, pad; };
int launch_piece_commit_frames(hipStream_t s, const PieceStage& st, const PieceCommitRec* recs_dev, const PieceCommitRec* host, int n, const int* table_dev, size_t table_ints,
                               unsigned long long* slab, size_t slab_words, uint8_t* piece_of, size_t piece_of_bytes);
// the capacities above for a test: contours, chain points (first level), contours, chain points (second level), piece slots, planes per frame
static inline void piece_capacities(int out[6]) { out[0] = PIECE_CONTOUR_CAP; out[1] = PIECE_CHAIN_CAP; out[2] = PIECE_CONTOUR_CAP2; out[3] = PIECE_CHAIN_CAP2; out[4] = PIECE_SLOTS; out[5] = PIECE_KMAX; }

}  // namespace sind
