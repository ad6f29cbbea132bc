// DynaDetect engine interface: state-free GPU front (gray, 0.6 resize, dense flow, up-scale) and the stateful
// per-stream tail (k-means, depth edges, PEAC, split/merge re-clustering, residual thresholds, mask fusion).
#pragma once
#include <algorithm>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "common.hpp"
#include "depth.hpp"
#include "flow.hpp"
#include "peac_grow.hpp"
#include "host/host.hpp"
#include "host/pieces.hpp"
#include "pieces_dev.hpp"

namespace sind {

struct DynaConfig { int W = 640, H = 480; float fx = 0, fy = 0, cx = 0, cy = 0, depthScale = 5000.f; int device = 0; };

static inline double tick_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- state-free front for B frames at once (reference DynaDetect.cc:1386-1392 gray, :1033-1147 flow) ------------------
class DynaFront {
public:
    DynaConfig cfg; int fw = 0, fh = 0, maxB = 0; hipStream_t stream = nullptr;
    FlowEngine flow;
    // speculate: flow(n, n-1) -- the reference's second DeepFlow pass for large-motion pairs (DD:1121-1131) -- is solved TOGETHER with flow(n, n-2), as the second half of
    // one batch of 2 B pairs, and the large-motion test then only picks between the two results.  For a batch that leaves most of the chip idle (one camera) the second
    // half costs next to nothing and a large-motion frame no longer takes two flow latencies in a row.  Same bits: a pair's flow does not depend on its batch.  Needs 2 B <= maxB.
    bool speculate = false;
    int init(const DynaConfig& c, int maxB, hipStream_t s);
    // bgr: device u8 [n][H][W][3] -> gray [n][H][W] and grayMin [n][fh][fw] (both device, caller-owned)
    int gray_and_min(const uint8_t* bgr, int n, uint8_t* gray, uint8_t* grayMin);
    // Dense flow for B pairs.  pool: device u8 frames [*][fh][fw]; cur/prev1/prev2: HOST index arrays into the pool
    // (frame n, n-1, n-2 of each pair).  U/V: device f32 [B][H*W] full-resolution flow (negated, refined, *1/0.6).
    // large_motion (host, optional): per-pair flag of the reference's second DeepFlow pass.
    int dense_flow(const uint8_t* pool, const int* cur, const int* prev1, const int* prev2, int B, float* U, float* V, int* large_motion,
                   float* dbg_deep_u = nullptr, float* dbg_deep_v = nullptr, float* dbg_ref_u = nullptr, float* dbg_ref_v = nullptr);
private:
    DevBuf<uint8_t> g0, g1; DevBuf<float> u, v, mag, u2, v2; DevBuf<unsigned> maxbits; DevBuf<int> hist, idx_dev;
    int gather(const uint8_t* pool, const int* idx_host, int B, uint8_t* out);
};

struct DynaDebug {           // stage outputs of the last tail call (parity tests)
    double H[9] = {0}; int nPairs = 0, hist[256] = {0}; float maxError = 0, otsu = 0, triangle = 0, thr_low = 0, thr_high = 0;
    std::vector<uint8_t> maskLow, maskHigh, kmeansLabel, occ1, occ2, totalArea, gradEdge, planeContours;
    float centers[KM_K][3] = {{0}}; int nClusters = 0;
};

struct OccResult { BitImg totalArea, occ1, occ2; bool ready = false; const float* gridFlow = nullptr;
                   uint8_t* occ2_dev = nullptr; uint8_t* depthN_dev = nullptr; hipEvent_t occ2_event = nullptr; };          // optional device slots the producer fills: plane-edge mask and 8-bit normalised depth for the RAG statistics     // state-free per-frame results computed ahead of the tail: CalOccluded outputs, flow at the 10-px sample grid (host)

// state of a frame between the two host halves of CalOccluded (the PEAC region grow runs on the GPU in between)
struct OccCtx { BitImg occ, totalArea; std::vector<PtI> endPoints; std::unique_ptr<PeacFitter> fit; bool grown_on_host = false;
                std::vector<int8_t> m8; std::vector<int16_t> m16; std::vector<uint8_t> pairs; };

// ---- GPU half of CalOccluded for a chunk of frames at once (state free: depth only).  Host-side results of one frame: OccGpuOut.
struct OccGpuOut { const uint8_t* edge; const uint8_t* total; const PeacBlockStats* blocks;
                   uint8_t* occ2_stage = nullptr; hipEvent_t occ2_event = nullptr; };      // optional: page-locked N bytes for the occ2 upload and the event recorded behind it
// The one statement of that half: the device workspaces for up to `cap` frames and the launches.  Frames at depth_dev + b * W * H; maxima of the filtered frames in
// umax[0, cap), of the raw frames (taken for the normalisation only) in umax[cap, 2 * cap).  Launches only (and the maxima's fills): no copy back, no wait, no allocation.
struct OccFront {
    DynaConfig cfg; int cap = 0;
    DevBuf<uint16_t> filt; DevBuf<uint8_t> edge, edgeTmp, total; DevBuf<unsigned> umax; DevBuf<PeacBlockStats> blocks;
    int init(const DynaConfig& c, int cap, bool block_stats = true);      // block_stats = false: no PEAC block statistics wanted (the parity entry, which has no intrinsics)
    // in two parts for whoever wants the edge before its opening: depthN_dev != nullptr: raw maximum + 8-bit normalised depth; then median 5, maximum, gradient edge + valid area ...
    int enqueue_edge(hipStream_t s, const uint16_t* depth_dev, int B, uint8_t* depthN_dev) const;
    // ... MORPH_OPEN with element4 (erode, dilate) and the PEAC block statistics
    int enqueue_open(hipStream_t s, const uint16_t* depth_dev, int B) const;
    int enqueue(hipStream_t s, const uint16_t* depth_dev, int B, uint8_t* depthN_dev) const { SIND_TRY(enqueue_edge(s, depth_dev, B, depthN_dev)); return enqueue_open(s, depth_dev, B); }
};
struct OccBatch {
    OccFront front;
    int init(const DynaConfig& c, int chunk) { return front.init(c, chunk); }
    // frames at depth_dev + b * W * H; outputs (host, page-locked): edge / valid-area masks and block statistics per frame; depthN_dev (device, optional)
    int run(hipStream_t s, const uint16_t* depth_dev, int B, uint8_t* depthN_dev, uint8_t* edge_h, uint8_t* total_h, PeacBlockStats* blocks_h);
};

// ---- stateful tail of one stream (reference DynaDetect.cc:1377-1666 minus the dense flow) ---------------------------------
// Output of the flow-independent half of a frame (k-means on the depth, CalOccluded, SegAndMerge): everything the flow-dependent
// half (flow masks, fusion) needs from it.  The pipeline computes it for all frames of a step while the dense flow is on the GPU.
struct DepthStageOut { std::vector<uint8_t> label3; int maxNum = 0; BitImg totalArea; bool ready = false; };

// ---- cv::kmeans of SegByKmeans (DD:315-420) for one frame of EVERY stream at once: the streams are independent, their per-frame chains of ~70
// small kernels are not worth a launch each (measured: 55 k launches per 512-pair step, the tails phase bound by their summed durations at a
// concurrency of ~2) -- one batched chain with blockIdx = (work, frame) does the same arithmetic with 1 / B of the launches.
struct KmFrameResult { const uint8_t* label8; float centers[KM_K][3]; int counts[KM_K]; };
// The one statement of the chain: the device workspaces for up to `cap` frames and the launches (depth pyramid; per level, coarsest first: points, labels -- the 3 x 4 grid or
// the resized previous labels at level 3, the resized coarser level below --, cv::kmeans; the u8 labels).  The caller puts the previous labels into labPrev8 and reads lab8 / kstate.
struct KmChain {
    int W = 0, H = 0, N = 0, cap = 0;
    DevBuf<uint16_t> dpyr[4]; DevBuf<float> px, py, pz, comp; DevBuf<int> lab[4], seg; DevBuf<uint8_t> labPrev8, lab8; DevBuf<KmState> kstate;
    int init(int W, int H, int cap);
    // frame b: device depth at depth_base + b * depth_stride.  use_prev_dev (device, one int per frame): both level-3 label kernels run and pick their frames by the flags;
    // nullptr: the one that use_prev_host names.  Launches only -- no copy, no wait, no allocation: the tail records the call into a HIP graph.
    int enqueue(hipStream_t s, const DynaConfig& cfg, const KmFuse& fuse, const uint16_t* depth_base, size_t depth_stride, int B, const int* use_prev_dev, bool use_prev_host) const;
};
class KMeansBatch {
public:
    int init(const DynaConfig& c, int maxB, hipStream_t s);
    // frame b: device depth at depth_base + b * depth_stride; prev[b] = the stream's previous merged labels (host u8 [H*W]) or nullptr for the
    // 3 x 4 grid start.  Blocks until the results are on the host; they stay valid until the next call.
    int run(const uint16_t* depth_base, size_t depth_stride, int B, const uint8_t* const* prev);
    const KmFrameResult& result(int b) const { return res[b]; }
    hipStream_t stream = nullptr;
    KmFuse km_fuse = g_km_fuse_default;      // copied when the object is made; never changes afterwards
private:
    DynaConfig cfg; int N = 0, maxB = 0;
    KmChain km; DevBuf<int> use_prev_d;
    PinnedBuf<uint8_t> h_prev, h_lab8; PinnedBuf<KmState> h_state; PinnedBuf<int> h_use_prev;
    std::vector<KmFrameResult> res;
};

// masks of one frame made ahead of its tail by the batched flow-mask stage: bit-packed in BitImg's layout, and the 261-word result block
// (histogram, maximum, thresholds lo / hi / otsu / triangle); page-locked host memory of the FlowMaskBatch that made them
struct FlowMasksReady { const uint64_t* low; const uint64_t* high; const int* res; };

class DynaTail;
// ---- GPU part of the flow-mask stage (DD:1252-1367: residual against the homography, u8 normalisation + histogram, Otsu / Triangle thresholds, both masks) for one
// frame of EVERY stream of a k-means group in four launches and one D2H: per frame it was four launches of 3.7 MB passes, a 615 KB copy and
// a stream wait, 512 times a step.  The masks come back bit-packed (77.8 KB per 640 x 480 frame), so the host packing is gone too.  Same arithmetic, same kernels'
// device functions; the residual workspaces and the working histogram stay the tails' own.
class FlowMaskBatch {
public:
    int init(const DynaConfig& c, int cap, hipStream_t s);
    ~FlowMaskBatch();
    int set(int b, DynaTail* tail, const float* U, const float* V, const double Hm[9]);      // record b (host side only; any thread, one per slot)
    int enqueue(int n);                       // records 0 .. n - 1: table upload, four launches, one D2H, the event
    int wait();                               // until the results are on the host; they stay valid until the next enqueue
    FlowMasksReady result(int b) const { const uint64_t* o = reinterpret_cast<const uint64_t*>(out_h.p) + slot_words * b; const size_t words = (size_t)H * (W / 64);
                                          return FlowMasksReady{o, o + words, reinterpret_cast<const int*>(o + 2 * words)}; }
    int capacity() const { return cap; }
    hipStream_t stream = nullptr;
private:
    DynaConfig cfg; int W = 0, H = 0, cap = 0, pending = 0; size_t slot_words = 0;
    PinnedBuf<FlowMaskRec> recs_h; DevBuf<FlowMaskRec> recs_d; DevBuf<unsigned long long> out_d; PinnedBuf<unsigned long long> out_h;
    std::vector<DynaTail*> tails; hipEvent_t done = nullptr;
};

// ---- GPU stage of SegAndMerge (DD:760-ish: the region-adjacency statistics over the pieces' bit planes) for one frame of EVERY stream of a k-means group, in chunks:
// per frame it was two plane uploads, two small launches of 128 workgroups that mostly zero and flush their counters, a copy back and a stream wait, 512 times a
// step.  A frame reserves a slot and plane space (any pool thread), packs its planes straight into the page-locked slab and joins; slots are handed out in order and
// chunk c holds slots [c * chunk, (c + 1) * chunk), so a chunk's planes, records and results are contiguous: one H2D of the planes, one of the records, two launches
// (launch_rag_frames), one D2H, one event.  Same kernels' device functions as the per-frame stage, integer counts: the same numbers.
class RagBatch {
public:
    int init(const DynaConfig& c, int max_frames, hipStream_t s);      // (cheap: the slabs are made by the first round that uses them)
    ~RagBatch();
    // chunk: frames per set of launches; planes_per_frame: the slabs hold max_frames * planes_per_frame input planes (2 per piece).  Not while a round is running.
    void set_limits(int chunk, int planes_per_frame) { chunk_n = chunk < 1 ? cap : std::min(chunk, cap); planes_frame = std::max(0, planes_per_frame); }      // (chunk < 1: the whole group)
    int chunk_frames() const { return chunk_n; }
    int begin_round();                                                 // forget the previous round's slots (whose results are no longer needed)
    // a slot and plane space for a frame of C pieces: *pieces and *conn take C planes each.  false: the slabs are full (the frame takes the per-frame stage)
    bool reserve(int C, int* slot, unsigned long long** pieces, unsigned long long** conn);
    // The same for the frames of one piece chunk (PieceBatch) at once: n consecutive slots, so that the run is still one set of launches.  on_device[i]: the frame's planes
    // are written into the DEVICE slab by the commit kernels (at plane_off(slot)) and no H2D covers them; else pieces[i] / conn[i] point into the page-locked slab as above.
    // slots[i] = -1: the slabs had no room for frame i (the others still form a run).  Returns the first slot handed out (-1: none).
    int reserve_run(int n, const int* C, const uint8_t* on_device, int* slots, unsigned long long** pieces, unsigned long long** conn);
    size_t plane_off(int slot) const { return recs_h.p[slot].plane_off; }
    unsigned long long* slab_dev() { return in_d.p; }
    size_t slab_words() const { return in_cap; }
    // slots [first, first + n) as one set of launches; its results are there after wait(ev) (ev < the capacity; enqueue(chunk) = the chunk's slots with ev = chunk)
    int enqueue_run(int first, int n, int ev);
    void set_inputs(int slot, const uint8_t* occ2, const uint8_t* depthN, hipEvent_t occ2_event);      // occ2_event: recorded behind the frame's occ2 upload on another stream (or nullptr)
    int chunk_of(int slot) const { return slot / chunk_n; }
    int chunk_first(int chunk) const { return chunk * chunk_n; }
    int chunk_count(int chunk) const { return std::max(0, std::min(chunk_n, n_slots - chunk * chunk_n)); }      // (of the slots handed out so far)
    int slots() const { return n_slots; }
    int enqueue(int chunk);                   // every slot of the chunk has been packed
    int wait(int chunk);                      // until the chunk's results are on the host; they stay valid until the next begin_round
    const int* result(int slot) const { return res_h.p + recs_h.p[slot].res_off; }
    hipStream_t stream = nullptr;
private:
    DynaConfig cfg; int W = 0, H = 0, cap = 0, chunk_n = 32, planes_frame = 64, n_slots = 0; size_t pw = 0, in_used = 0, res_used = 0, in_cap = 0, res_cap = 0;
    std::mutex m, enq;
    PinnedBuf<unsigned long long> in_h; DevBuf<unsigned long long> in_d, dil_d; PinnedBuf<RagRec> recs_h; DevBuf<RagRec> recs_d; DevBuf<int> res_d; PinnedBuf<int> res_h;
    std::vector<hipEvent_t> occ2_ev, done; std::vector<uint8_t> on_dev;      // on_dev: the slot's planes lie in the device slab already
    bool reserve_locked(int C, bool dev, int* slot, unsigned long long** pieces, unsigned long long** conn);
};

// ---- SegAndMerge's piece extraction (DD:664-729) for one frame of EVERY stream of a k-means group, in chunks: one PieceStage (pieces_dev.hpp) of capacity `chunk` in
// front of the RagBatch's join, its commit writing straight into the RagBatch's device slab.  Per tail the stage was a chain of 13 + 2 launches of mostly one-wave
// kernels with two waits (profiles/seg_pieces.txt); here a chunk is ONE such chain.  A frame takes a slot (any pool thread) and packs its inputs into the page-locked
// slab; slots are handed out in order and chunk c holds slots [c * chunk, (c + 1) * chunk).  enqueue(chunk): the chunk's inputs up (cluster planes, occ1,
// labelForSegEdge, plane counts, depth table: five copies, each contiguous over the chunk), the 13 launches, frame headers and records down, one event.  After the host
// step (seg_pieces_order per frame, host/pieces.hpp) commit(chunk) sends the order tables up and launches k_piece_commit_frames / k_piece_paint_frames for the frames
// that stayed on the device, and brings their pieceOf back on the same stream: whoever waits for the RAG launches behind it has pieceOf too.
// Capacity: the chunk is at most 64 frames (PieceStage::init), whatever the RAG chunk setting says.
// Workspaces (made by the first round that uses them; an allocation failure is returned with its text, nothing else is tried).  With pw = H * W / 64 words per plane:
//   4 plane sets of PIECE_SLOTS planes per frame           chunk * 4 * 255 * pw * 8 bytes      640 x 480, chunk 32: 1.25 GB
//   3 sets of PIECE_KMAX planes + 3 planes per frame       chunk * 39 * pw * 8                 48 MB
//   first-level tracer (12 planes per frame)               chunk * 12 * (1024 * 40 + 32768 * 4) 66 MB
//   second-level tracer (255 planes per frame)             chunk * 255 * (256 * 40 + 16384 * 4) 0.62 GB
//   the stage's own depth planes (unused here), records    chunk * (W * H * 2 + 255 * 72)      20 MB
//   above 144 KB of mark cells per plane (1280 x 720)      chunk * 267 * (W + 2)(H + 2) / 4    (global scratch: 1.98 GB at 1280 x 720, none at 640 x 480)
//   per frame of the GROUP: input slab 14 planes (page-locked), pieceOf W * H (device and page-locked), records 16 KB, tables 2 KB
// i.e. about 2.0 GB at 640 x 480 and chunk 32 (1.25 GB of it the four plane sets, 0.62 GB the second-level tracer); at 1280 x 720 the plane sets are three times
// as large (3.8 GB), the tracers stay, and the scratch cells come on top: about 6.6 GB.  One object per k-means group.
class PieceBatch {
public:
    int init(const DynaConfig& c, int max_frames, hipStream_t s);      // (cheap: the workspaces are made by the first round that uses them)
    ~PieceBatch();
    void set_chunk(int chunk) { chunk_n = std::max(1, std::min(chunk < 1 ? cap : chunk, std::min(cap, 64))); }      // not while a round is running
    int chunk_frames() const { return chunk_n; }
    int begin_round();                                                 // workspaces on first use; forget the previous round's slots
    int take_slot();                                                   // -1: every slot of the group is taken
    // the frame's inputs into its slot: nCl (1 .. PIECE_KMAX) cluster planes, occ1, labelForSegEdge, where its depth plane lies on the device
    void pack(int slot, const BitImg* labels, int nCl, const BitImg& occ1, const BitImg& label_edge, const uint16_t* depth_dev);
    int chunk_of(int slot) const { return slot / chunk_n; }
    int chunk_first(int chunk) const { return chunk * chunk_n; }
    int chunk_count(int chunk) const { return std::max(0, std::min(chunk_n, n_slots - chunk * chunk_n)); }
    int slots() const { return n_slots; }
    int enqueue(int chunk, int z_invalid_from, float inv_depth_scale);
    int wait(int chunk);
    const PieceFrameHdr& header(int slot) const { return hdr_h.p[slot]; }
    const PieceRecDev* records(int slot) const { return recs_h.p + (size_t)slot * PIECE_SLOTS; }
    int* order_table(int slot) { return tab_h.p + (size_t)slot * 2 * PIECE_SLOTS; }      // [0, PIECE_SLOTS): slot per rank; [PIECE_SLOTS, 2 PIECE_SLOTS): has_conn per rank
    // frames `slots[i]` of the chunk (C[i] ranked pieces, order tables filled) into `slab` at plane_off[i]: tables up, two launches, pieceOf down.  No wait
    int commit(int chunk, int n, const int* slots, const int* C, const size_t* plane_off, unsigned long long* slab, size_t slab_words);
    const uint8_t* piece_of(int slot) const { return pof_h.p + (size_t)slot * N; }
    std::mutex& flush_mutex() { return flush_mu; }      // one chunk at a time from its piece launches to its commit launches: the stage's planes are the chunk's until then
    const PieceStage& stage() const { return st; }
    hipStream_t stream = nullptr;
private:
    DynaConfig cfg; int W = 0, H = 0, cap = 0, chunk_n = 32, n_slots = 0; size_t pw = 0, N = 0; bool ready = false;
    std::mutex m, flush_mu;
    PieceStage st; DevBuf<const uint16_t*> dtab_d; DevBuf<uint8_t> pof_d; DevBuf<PieceCommitRec> crec_d; DevBuf<int> tab_d;
    PinnedBuf<unsigned long long> planes_h, occ1_h, edge_h; PinnedBuf<int> np_h; PinnedBuf<const uint16_t*> dtab_h;      // per slot: PIECE_KMAX planes, occ1, labelForSegEdge, plane count, depth pointer
    PinnedBuf<PieceFrameHdr> hdr_h; PinnedBuf<PieceRecDev> recs_h; PinnedBuf<int> tab_h; PinnedBuf<PieceCommitRec> crec_h; PinnedBuf<uint8_t> pof_h;
    std::vector<hipEvent_t> done;
};
// One frame of a chunk through the flush below: its depth-half tail (in), and what became of it (out): rc / err != OK: the frame failed (more than 254 pieces) and
// nothing else holds; rag_slot >= 0: its counters are rb.result(rag_slot) after the flush; rag_slot < 0 with pieces: the slab had no room, it takes the per-frame stage
// (own); on_device: its planes were committed on the device and its pieceOf is pb.piece_of(slot)
struct PieceChunkFrame { DynaTail* half = nullptr; int rc = 0; std::string err; int rag_slot = -1; bool own = false, on_device = false, fell_back = false; };
// The flush of one piece chunk, stated once for the pipeline and the parity entry: piece launches, wait, the host step of every frame (a frame whose status is not 0
// runs the host function here and is packed from the host: the run may mix both kinds), reservation of the run, commit and paint launches, RAG launches, wait.
// fr: chunk_count(chunk) frames in slot order.  A failure returned is the chunk's: every frame of it has failed.
int piece_chunk_flush(PieceBatch& pb, RagBatch& rb, int chunk, PieceChunkFrame* fr);

class DynaTail {
public:
    DynaConfig cfg; hipStream_t stream = nullptr; DynaDebug dbg; bool keep_debug = false;
    KmFuse km_fuse = g_km_fuse_default;      // copied when the object is made; never changes afterwards
    // SegAndMerge's piece extraction on the GPU (PieceStage of pieces_dev.hpp at capacity 1, on this tail's stream) instead of the host function; off by default.  Same pieces
    // in the same order, bit for bit; a frame in which a plane exceeds a capacity of the device stage runs the host function and counts as fallen back.  The workspaces
    // are made by the first frame that takes the path.
    bool device_pieces = false; long long n_pieces_device = 0, n_pieces_fallback = 0;
    int piece_threads = 1;        // host threads for the per-cluster piece extraction of SegAndMerge (> 1 only when host cores idle: a single stream in the in-order mode)
    int init(const DynaConfig& c, hipStream_t s);
    ~DynaTail() { for (auto& g : kmGraph) if (g) (void)hipGraphExecDestroy(g); }
    // depth_host: H x W u16 (host); depth_dev: same on the device; U/V: device full-resolution flow of this frame.
    // dyna_out / label_out: host H x W u8 (0 invalid / 125 static / 255 dynamic ; 0 invalid, 1..n clusters).
    // depth_half: the tail object that carries the depth half's state and workspaces (nullptr = this one)
    int process(const uint16_t* depth_host, const uint16_t* depth_dev, const float* U, const float* V, uint8_t* dyna_out, uint8_t* label_out,
                const OccResult* precomputed = nullptr, DynaTail* depth_half = nullptr, const KmFrameResult* km = nullptr, const FlowMasksReady* fm = nullptr);
    // host part of the flow-mask stage (DD:1163-1250): sample weights from the state the previous frame left, PROSAC order, pairs, homography.  The batched
    // stage calls it for every stream of a group before ONE set of launches (FlowMaskBatch); fills dbg.nPairs / dbg.H
    int flow_masks_homography(const float* U, const float* V, const float* gridFlowPre, double Hm[9]);
    // the k-means warm labels of the next frame (nullptr before the first frame of a stream): what KMeansBatch::run wants as prev[b]
    const uint8_t* prev_km_labels() const { return kmLabelLastAny ? kmLabelLast.data() : nullptr; }
    // process() in two parts around the batched RAG stage (RagBatch): process_begin runs the frame up to SegAndMerge's pieces, process_end takes the counters and does
    // the rest.  Between them, on the depth-half object (rag_half()): rag_pieces() pieces (0: nothing to count, process_end(nullptr)); rag_batchable(): occ2 and the
    // normalised depth are on the device already; rag_pack() writes the piece and connection planes; rag_own() is the per-frame stage.  Same arithmetic in the same order.
    int process_begin(const uint16_t* depth_host, const uint16_t* depth_dev, const float* U, const float* V, const OccResult* precomputed, DynaTail* depth_half,
                      const KmFrameResult* km, const FlowMasksReady* fm);
    // piece_of: the frame's pieceOf where a PieceBatch painted it (seg_pieces_batched from records), else nullptr
    int process_end(const int* rag, uint8_t* dyna_out, uint8_t* label_out, const uint8_t* piece_of = nullptr);
    // process_begin in two parts around a round's batched piece stage (PieceBatch): process_begin_inputs runs the frame up to the INPUTS of SegAndMerge's piece
    // extraction (on rag_half(): piece_labels() -- the last one is the farthest cluster, which is not cut --, piece_occ1(), piece_edge(), piece_depth_dev());
    // seg_pieces_batched() is the rest of process_begin from the frame's records (ranked: seg_pieces_order) or, with recs = nullptr, through the host function.
    // piece_batchable(): the frame has 1 .. PIECE_KMAX clusters to cut and its depth, occ2 and normalised depth are on the device.  process_begin = both parts, the
    // second through seg_pieces.  order / has_conn: PIECE_SLOTS ints each (the commit kernels' table).  SIND_E_CAPACITY: more than 254 pieces, as on every path.
    int process_begin_inputs(const uint16_t* depth_host, const uint16_t* depth_dev, const float* U, const float* V, const OccResult* precomputed, DynaTail* depth_half,
                             const KmFrameResult* km, const FlowMasksReady* fm);
    bool piece_batchable() const { const int nCl = (int)segLabels.size() - 1; return nCl >= 1 && nCl <= PIECE_KMAX && segDepthDev && segPre && segPre->occ2_dev && segPre->depthN_dev; }
    const std::vector<BitImg>& piece_labels() const { return segLabels; }
    const BitImg& piece_occ1() const { return segOcc1; }
    const BitImg& piece_edge() const { return segEdge; }
    const uint16_t* piece_depth_dev() const { return segDepthDev; }
    int seg_pieces_batched(const PieceRecDev* recs, int C, int* order, int* has_conn);
    int piece_z_invalid_from() const { return zInvalidFrom; }
    float piece_inv_depth_scale() const { return invDepthScale; }
    // parity-test access (sind_debug_pieces_batch): a frame's piece inputs as process_begin_inputs leaves them, and its pieces afterwards
    void debug_set_piece_inputs(const unsigned long long* planes, int k, const unsigned long long* occ1, const unsigned long long* label_edge, const uint16_t* depth_host,
                                const uint16_t* depth_dev, const OccResult* pre);
    const std::vector<SegPiece>& debug_pieces() const { return segAll; }
    const std::vector<uint8_t>& debug_piece_of() const { return segPieceOf; }
    DynaTail* rag_half() { return pendHalf ? pendHalf : this; }
    int rag_pieces() const { return (int)segAll.size(); }
    bool rag_batchable() const { return !segOnDevice && segPre && segPre->occ2_dev && segPre->depthN_dev; }      // (pieces cut on the device stay there: RagBatch takes host planes, such a frame runs rag_own)
    const OccResult* rag_pre() const { return segPre; }
    void rag_pack(unsigned long long* pieces, unsigned long long* conn) const;
    int rag_own(const int** rag);
    // process() = depth_stage() + flow_stage().  The two halves keep separate state (the k-means warm labels belong to the depth half,
    // the sample weights / previous masks to the flow half), so the depth half of the next frames may run ahead of the flow half.
    // km: this frame's k-means result when it was computed by the batched chain (else the stage runs its own)
    int depth_stage(const uint16_t* depth_host, const uint16_t* depth_dev, const OccResult* precomputed, DepthStageOut& out, const KmFrameResult* km = nullptr);
    // fm: this frame's masks when the batched flow-mask stage made them (else the stage runs its own launches)
    int flow_stage(const float* U, const float* V, const DepthStageOut& d, uint8_t* dyna_out, uint8_t* label_out, const float* gridFlowPre = nullptr, const FlowMasksReady* fm = nullptr);
    // CalOccluded (DD:429-642) depends on the depth frame only: the pipeline runs it on this tail's stream while the dense flow
    // of the step is still on the GPU and the host cores are idle
    int compute_occluded(const uint16_t* depth_host, const uint16_t* depth_dev, OccResult& out, const OccGpuOut* pre = nullptr);
    // the same in two halves around a batched launch of the PEAC region grow (peac_grow.hpp): grow_block = the frame's page-locked input block
    int compute_occluded_p1(const uint16_t* depth_host, const uint16_t* depth_dev, OccCtx& c, const OccGpuOut* pre, uint8_t* grow_block, int depth_index);
    int compute_occluded_p2(OccCtx& c, const int8_t* member8, const uint8_t* pair_seen, const int* grow_status, OccResult& out, const OccGpuOut* pre);
    long n_grow_fallback = 0;      // frames whose region grow overflowed a capacity of the kernel and ran on the host
    void reset();
    // Inter-frame state (reference DynaDetect.h:172-178, rolled at DynaDetect.cc:1660-1664) as one flat blob, so that a sequence can
    // continue on another handle / rank exactly where this one stopped ("phase B strictly in frame order"):
    //   [dynaLast N][labelLast N][highLast N (0/255)][lastCnt 256 x i32][lastDyn 256 x i32]   flow half (sample weights, previous high mask)
    //   [kmLabelLast N][kmLabelLastAny i32]                                                  depth half (k-means warm labels)
    size_t state_bytes() const { return (size_t)4 * N + 2 * 256 * sizeof(int) + sizeof(int); }
    void save_state(uint8_t* buf, bool flow_half = true, bool depth_half = true) const;
    void load_state(const uint8_t* buf, bool flow_half = true, bool depth_half = true);
    // hash_state: leave a 128-bit fingerprint of the rolled state (host/statehash.hpp) in state_hash after every frame -- what the chunked sequence mode
    // compares at the chunk seams (sind_pipe_set_state_hashing).  It covers everything the blob carries: the blob's other fields are functions of these images.
    bool hash_state = false; uint64_t state_hash[2] = {0, 0};
    double t_stage[6] = {0, 0, 0, 0, 0, 0}; long n_frames = 0;
    double t_fine[40] = {0};       // cal_occluded: gpu+d2h, pack, endpoints, peac, contour filter, close | seg_merge: pieces, planes+h2d, rag gpu, merge    // flow masks, k-means, label prep, CalOccluded, SegAndMerge, fusion (ms, SIND_TAIL_TIMING=1)
private:
    friend class FlowMaskBatch;       // its records point at this tail's residual workspaces (mag, magu8, hist_d) and it keeps hist_clean
    int W = 0, H = 0, N = 0, zInvalidFrom = 65536; float invDepthScale = 0.f;
    std::vector<uint8_t> dynaLast, labelLast; BitImg highLast;       // host state images (DynaDetect.h:172-178) as seen by the flow half
    int lastCnt[256] = {0}, lastDyn[256] = {0};
    std::vector<uint8_t> kmLabelLast; bool kmLabelLastAny = false;   // imgLabelLast as seen by the depth half (k-means warm labels, DD:374-395)
    // device workspaces
    KmChain km; OccFront occ;       // the k-means chain and the GPU front of CalOccluded, one frame each
    DevBuf<uint8_t> depthN, occ2_d, magu8, low_d; DevBuf<unsigned long long> planes_d; DevBuf<int> hist_d, rag_d; DevBuf<float> mag, grid_d;
    // page-locked staging of everything that crosses PCIe in a tail
    PinnedBuf<float> h_grid; PinnedBuf<int> h_hist, h_rag; PinnedBuf<uint8_t> h_ab, h_lab8; PinnedBuf<KmState> h_kstate; PinnedBuf<PeacBlockStats> h_blocks;
    PinnedBuf<unsigned long long> h_planes;
    int flow_masks(const float* U, const float* V, BitImg& low, BitImg& high, const float* gridFlowPre = nullptr);
    int flow_masks_gpu(const float* U, const float* V, const double Hm[9]);      // residual, histogram, thresholds, u8 masks; one D2H into h_ab, one wait
    void flow_masks_result(const int* res261);
    void flow_masks_ready(const FlowMasksReady& fm, BitImg& low, BitImg& high);
    int fuse(const BitImg& maskLow, const BitImg& maskHigh, const DepthStageOut& d, uint8_t* dyna_out, uint8_t* label_out);
    int kmeans(const uint16_t* depth_dev, std::vector<uint8_t>& label8, float centers[KM_K][3], int counts[KM_K]);
    bool hist_clean = false;      // hist_d's working block is known to be zero (left so by k_flow_thresholds)
    DevBuf<uint16_t> depth_fix; hipGraphExec_t kmGraph[2] = {nullptr, nullptr}; bool kmGraphBroken = false;
    // depthN_dev (optional, only without `pre`): the 8-bit normalised depth rides ahead of the edge chain (OccFront)
    int cal_occluded(const uint16_t* depth_host, const uint16_t* depth_dev, BitImg& totalArea, BitImg& occ1, BitImg& occ2, const OccGpuOut* pre = nullptr, uint8_t* depthN_dev = nullptr);
    int cal_occluded_p1(const uint16_t* depth_host, const uint16_t* depth_dev, OccCtx& c, const OccGpuOut* pre, uint8_t* grow_block, int depth_index, uint8_t* depthN_dev = nullptr);
    int cal_occluded_p2(OccCtx& c, const int8_t* member8, const uint8_t* pair_seen, const int* grow_status, BitImg& occ1, BitImg& occ2);
    int finish_occluded(OccResult& out, const OccGpuOut* pre);
    struct OwnGrow { PeacGrowBatch batch; PinnedBuf<uint8_t> in_h, pair_h; PinnedBuf<int8_t> member_h; PinnedBuf<int> status_h; };
    std::unique_ptr<OwnGrow> own_grow;         // one-frame grow workspace, created on first use (single-frame API, unbatched pipeline steps)
    // SegAndMerge (DD:644-1031) in three parts: the host part up to the sorted pieces and pieceOf (seg_pieces), the GPU stage (rag_pack + seg_rag_gpu per frame, or a
    // RagBatch), the host part from the counters on (seg_finish).  The pieces (areas, hasLianjie, images until they are packed), pieceOf and what the per-frame stage
    // needs live here in between; depth_stage() = depth_stage_begin + seg_rag_gpu + depth_stage_end
    std::vector<SegPiece> segAll; std::vector<uint8_t> segPieceOf; BitImg segOcc1, segOcc2; const uint16_t* segDepthDev = nullptr; const OccResult* segPre = nullptr;
    BitImg pendLow, pendHigh; DepthStageOut pendD; DynaTail* pendHalf = nullptr;      // process_begin -> process_end
    int depth_stage_begin(const uint16_t* depth_host, const uint16_t* depth_dev, const OccResult* precomputed, DepthStageOut& out, const KmFrameResult* km);
    // depth_stage_begin = depth_stage_inputs (up to the inputs of the piece extraction, kept in segLabels / segOcc1 / segEdge / segDepthHost) + depth_stage_pieces
    std::vector<BitImg> segLabels; BitImg segEdge; const uint16_t* segDepthHost = nullptr;
    int depth_stage_inputs(const uint16_t* depth_host, const uint16_t* depth_dev, const OccResult* precomputed, DepthStageOut& out, const KmFrameResult* km);
    int depth_stage_pieces();
    int seg_pieces_check_and_rank(bool on_device);      // the rest of seg_pieces once segAll holds the pieces in discovery order
    int depth_stage_end(DepthStageOut& out, const int* rag);
    int seg_pieces(const std::vector<BitImg>& allLabels, const BitImg& occ1, const BitImg& labelForSegEdge, const uint16_t* depth_host, bool allow_device = true);
    int seg_rag_gpu(const int** rag);
    std::unique_ptr<PieceStage> pieceStage; PinnedBuf<unsigned long long> h_pieceIn, h_pieceOut; PinnedBuf<PieceRecDev> h_pieceRecs; PinnedBuf<PieceFrameHdr> h_pieceHdr; PinnedBuf<int> h_pieceNp;
    int seg_pieces_device(const std::vector<BitImg>& allLabels, const BitImg& occ1, const BitImg& labelForSegEdge, std::vector<SegPiece>& all, bool* done);      // dyna_pieces.cpp
    bool segOnDevice = false;      // this frame's pieces were cut on the device: segAll holds their records only, the planes lie in planes_d (rank order), pieceOf in pieceOf_d
    DevBuf<uint8_t> pieceOf_d; DevBuf<int> pieceOrder_d; PinnedBuf<int> h_pieceOrder; PinnedBuf<uint8_t> h_pieceOf;
    int seg_pieces_commit();       // dyna_pieces.cpp: the rank order up, k_piece_commit
public:
    // parity-test access (sind_debug_seg_pieces, n = 1): this tail's own piece path -- switch, capacity-1 stage on its stream, fallback, ranking, commit -- on given planes.
    // k cluster planes (all are cut), depth_dev on the device.  Afterwards `out` holds the pieces in RANK order with their planes and pieceOf, wherever they were made
    int debug_seg_pieces(const unsigned long long* planes, int k, const unsigned long long* occ1, const unsigned long long* label_edge, const uint16_t* depth_host, const uint16_t* depth_dev,
                         std::vector<SegPiece>& out, std::vector<uint8_t>& piece_of);
private:
    void seg_finish(const int* rag, std::vector<uint8_t>& labelNew);
};

}  // namespace sind
