#pragma once
// Batched multi-stream pipeline (include/sind_hip.h "sind_pipe"): the frame-loop body of the reference's
// Examples/RGB-D/rgbd_tum_noros.cc:110-170 (DetectDynaArea -> 15x15 dilate -> ORBextractor via Frame::ExtractORB2) for
// S independent streams x T frames per step.
//   phase A (state free, one batch of S*T frames on the shared HIP stream): gray, 0.6 resize, dense flow, ORB front
//   phase B (stateful, frame order inside a stream; one task per frame on a fixed worker pool, one HIP stream per worker):
//            DynaDetect tail, dilation, dynamic-mask erasure of the ORB keypoints.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <sched.h>
#include <ctime>
#include <cstdio>
#include "../../include/sind_hip.h"
#include "dyna.hpp"
#include "orb.hpp"
#include "pipeline_pool.hpp"
#include "host/pipe_schedule.hpp"

using namespace sind;

// CPU time (user + system) of the calling thread in ms, for the SIND_TAIL_TIMING report of the short-lived phase-A threads
static inline double thread_cpu_ms() { timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
inline std::atomic<long long> g_cpu_us_flow{0}, g_cpu_us_orb{0}, g_cpu_steps{0};

// First failure per slot (a stream, a frame, a flow slice).  A slot is written by the task that owns it, without a lock.
struct Failures {
    std::vector<int> rc; std::vector<std::string> err;
    void reset(int n) { rc.assign(n, SIND_OK); err.assign(n, std::string()); }
    bool ok(int i) const { return rc[i] == SIND_OK; }
    void fail(int i, int r, const std::string& e) { rc[i] = r; err[i] = e; }
    void fail(int i, int r) { fail(i, r, sind_last_error()); }
    void fail_all(int i0, int i1, int r, const char* prefix, const std::string& msg = sind_last_error()) {      /* slots that have not failed yet */ for (int i = i0; i < i1; i++) if (ok(i)) fail(i, r, prefix + msg); }
    // the first failed slot becomes the last error: fmt takes slot / per and the message
    int first_error(const char* fmt, int per = 1) const { for (int i = 0; i < (int)rc.size(); i++) if (!ok(i)) { sind_set_error(fmt, i / per, err[i].c_str()); return rc[i]; } return SIND_OK; }
};

// Phase-A outputs of a step, everything the tails read; a member of both step buffers and of every retained step, which change places by swap()
struct PhaseAOut {
    DevBuf<float> U, V; DevBuf<uint16_t> depth_dev; PinnedBuf<uint16_t> depth_h;       // (page-locked: the 157 MB device-to-host copy of a step must not block the enqueueing thread)
    DevBuf<uint8_t> occ2_dev, depthN_dev;                  // per frame: plane-edge mask and normalised depth for the tails' RAG statistics (filled by the CalOccluded tasks)
    DevBuf<float> grid_dev; PinnedBuf<float> grid_h;       // flow at the 10-px sample grid of every frame (DD:1182-1204), gathered right after the dense flow
    std::vector<OrbFrameResult> orb; std::vector<OccResult> occ;
    std::vector<int> large_motion;                         // per pair k = s * T + t: took the second DeepFlow pass (every flow slice writes its own range)
    // gsz = 0 (construction): flow and depth copies only -- the rest comes with the first step that fills this set
    int alloc(size_t np, size_t B, size_t gsz) {
        SIND_TRY(U.alloc(np * B)); SIND_TRY(V.alloc(np * B)); SIND_TRY(depth_dev.alloc(np * B)); SIND_TRY(depth_h.alloc(np * B));
        if (gsz == 0) return SIND_OK;
        SIND_TRY(occ2_dev.alloc(np * B)); SIND_TRY(depthN_dev.alloc(np * B)); SIND_TRY(grid_dev.alloc(gsz * B)); SIND_TRY(grid_h.alloc(gsz * B));
        return SIND_OK;
    }
    void swap(PhaseAOut& o) {
        U.swap(o.U); V.swap(o.V); depth_dev.swap(o.depth_dev); depth_h.swap(o.depth_h); occ2_dev.swap(o.occ2_dev); depthN_dev.swap(o.depthN_dev); grid_dev.swap(o.grid_dev); grid_h.swap(o.grid_h);
        orb.swap(o.orb); occ.swap(o.occ); large_motion.swap(o.large_motion);
    }
};

struct sind_pipe {
    sind_pipe_config c{}; DynaConfig dc; int S = 0, T = 0, fw = 0, fh = 0;
    size_t np() const { return (size_t)c.width * c.height; }      // pixels of a frame
    size_t gsz() const { return (size_t)2 * ((c.width - 1) / 10) * ((c.height - 1) / 10); }      // values of a frame's sample-grid flow
    hipStream_t stream = nullptr, orb_stream = nullptr; hipEvent_t ev_gray = nullptr, ev_depth = nullptr; std::vector<hipStream_t> worker_streams;      // one HIP stream per pool worker, shared by the tasks it runs
    DynaFront front; std::vector<std::unique_ptr<DynaFront>> extra_fronts; std::vector<hipStream_t> extra_streams; hipEvent_t ev_pool = nullptr;      // batch slices 1.. of the dense flow (slice 0 = front)
    OrbEngine orb; std::vector<std::unique_ptr<DynaTail>> tails;
    bool device_pieces = false;      // every stream's tail (and depth half) cuts its pieces on the GPU (DynaTail::device_pieces)
    // Depth halves (k-means warm labels + their workspaces) as objects of their own, present once depth-ahead has been switched on: the
    // depth chain of step i+1 (phase A) may then run while the flow chain of step i (phase B) is still going on the same stream of frames.
    std::vector<std::unique_ptr<DynaTail>> dtails;
    // k-means of one frame of every stream as ONE batched kernel chain (phase B then runs frame t of all streams as a round: batched k-means,
    // then the S tails of that frame on the pool); used when there are several streams and the depth half is not run ahead
    static constexpr int KM_GROUPS = 4;
    KMeansBatch kmb[KM_GROUPS]; int km_groups = 1, km_groups_max = 1, km_groups_fixed = -1; hipStream_t km_streams[KM_GROUPS] = {nullptr}; bool batch_km = false;
    // flow-mask stage of a round, batched the same way (FlowMaskBatch, dyna.hpp): in the non-split rounds every stream of a group holds the state its homography needs
    // once the round thread has waited for the previous round's tails, so the homographies are computed on the pool WHILE the batched k-means runs and the stage's
    // kernels run once for the group.  One set per handle: phase B of two steps is never in flight together (a submit finishes the previous step's tails before it returns).
    FlowMaskBatch fmb[KM_GROUPS]; bool fm_batch = true; std::atomic<long long> fm_frames{0};
    // RAG stage of SegAndMerge in the same rounds, batched per chunk of the group's frames (RagBatch, dyna.hpp; pipeline_frame.cpp: tail_rag_begin) on the group's k-means
    // stream, which is idle while the round's tails run.  rag_chunk: frames per set of launches (< 1: the whole group); rag_planes: input planes of slab per frame
    struct RagRound { std::mutex m; int expected = 0, arrived = 0; std::vector<int> joined, stream_of_slot; };      // frames of the round / through their first task, packed slots per chunk, whose slot
    RagBatch ragb[KM_GROUPS]; RagRound ragr[KM_GROUPS]; bool rag_batch = true; int rag_chunk = 32, rag_planes = 64; std::atomic<long long> rag_frames{0}, rag_fallback{0};
    // Piece extraction of SegAndMerge in the same rounds (PieceBatch, dyna.hpp; pipeline_frame.cpp: tail_pieces_begin), opt-in: one device stage per chunk of rag_chunk
    // (at most 64) frames in front of the RAG batch's join, on the same stream; the round's bookkeeping is the RAG round's (ragr)
    PieceBatch pieceb[KM_GROUPS]; bool pieces_batch = false; std::atomic<long long> pieces_frames{0}, pieces_fallback{0};
    std::vector<std::thread> round_threads; std::mutex km_stat_mu; double km_round_ms = 0; long km_rounds = 0;
    std::vector<std::unique_ptr<PinnedBuf<uint8_t>>> upload_stage;        // page-locked staging of sind_pipe_process (host-buffer entry point), two 4 MB buffers per uploading worker
    std::vector<std::unique_ptr<DynaTail>> occ_tails;     // CalOccluded workspaces, one per pool worker (state free)
    // GPU half of CalOccluded for all frames of a step, in chunks, on a stream of its own at the start of phase A (seven launches per chunk instead
    // of seven launches + a stream wait per frame); the runner tasks wait for their frame's chunk and do the host half
    OccBatch occb; hipStream_t occ_stream = nullptr; bool batch_occ = false; int occ_chunk = 64;
    // PEAC region grow of CalOccluded on the GPU, one launch per chunk of frames (peac_grow.hpp): the runner that finishes the last first-half of a chunk enqueues it
    PeacGrowBatch grow; hipStream_t grow_stream = nullptr; std::mutex grow_mu; bool grow_ok = false;       // grow_ok: the frame size fits the kernel (else every frame grows on the host)
    // Where a frame's region grow runs: grow_q of every 4 frames on the GPU (one CU for ~6 ms per frame), the others on the host (one core for ~5 ms); both give
    // the same bits, so the share only moves load.  grow_q_fixed < 0: adapted step by step (grow_adapt) -- towards the GPU while the step waits for host work
    // (CalOccluded or tails not done when the dense flow is), back towards the host while no step waits.
    // (the share starts with every grow on the GPU: measured in round 4, the controller ends there within a few steps at both sizes, and a run that starts there keeps the host two cores cooler at the same rate)
    int grow_q = 4, grow_q_fixed = -1, grow_idle_steps = 0; int cpu_share = 16; int host_info[6] = {0, 0, 0, 0, -1, 1};      // host_info: share, workers, tokens, cores usable, cgroup quota (-1 none), ranks of the node
    DevBuf<uint8_t> bgr_d, gray, gray_orb, pool; DevBuf<uint16_t> depth_d;
    // two sets of phase-A outputs: step i's phase A (GPU) overlaps with step i-1's phase B (host threads + small kernels)
    struct StepBuf {
        PhaseAOut a; bool pending = false;
        std::atomic<int> occ_next{0};                          // next frame for the CalOccluded runner tasks
        std::vector<OccCtx> occ_ctx; PinnedBuf<uint8_t> grow_in_h, grow_pair_h; PinnedBuf<int8_t> grow_member_h; PinnedBuf<int> grow_status_h;      // per frame: state between the halves, the grow's input block and results
        std::vector<hipEvent_t> grow_ev; std::unique_ptr<std::atomic<int>[]> grow_left, grow_state; std::atomic<int> occ_next2{0}; int grow_q = 4;      // per chunk: first halves still out, 0 = not launched / 1 = launched / < 0 = failed
        PinnedBuf<uint8_t> occ_edge_h, occ_total_h; PinnedBuf<PeacBlockStats> occ_blocks_h; std::vector<hipEvent_t> occ_ev, occ2_ev;      // batched GPU half: per-frame host results, one event per chunk; one event per frame behind its occ2 upload
        // depth half of the tails (k-means, SegAndMerge) run ahead, underneath the dense flow (synchronous steps only): per-frame results,
        // and a gate per frame that opens when both its CalOccluded result and the stream's previous depth stage are there
        bool depth_ahead = false; std::vector<DepthStageOut> dout; std::unique_ptr<std::atomic<int>[]> gate; TaskGroup depth_group;
        TaskGroup fm_group[KM_GROUPS];      // per k-means group: the homography tasks of a round's batched flow-mask stage
        TaskGroup occ_group, tail_group, km_tails[KM_GROUPS]; int km_groups = 1, km_first[KM_GROUPS + 1] = {0};       // the step's own partition of the streams
        Failures occ_fail, depth_fail, tail_fail, dchain_fail;      // per frame: CalOccluded, depth stage run ahead; per stream: tail, depth chain (two chains / split rounds: its flow chain writes tail_fail -- two workers, two slots)
        std::vector<int> active, first; std::vector<uint64_t> state_hash;      // tails of stream s run for first[s] <= t < active[s] (empty: 0 / all T); per-frame state fingerprints [S][T][2]
        // the frames [t0, t1) of stream s whose tails run in this step (set_active_frames and replay admit 0 <= first[s] and active[s] <= T only: no clamp)
        struct Frames { int t0, t1; };
        bool ragged() const { return !first.empty() || !active.empty(); } Frames range(int s, int T) const { return {first.empty() ? 0 : first[s], active.empty() ? T : active[s]}; }
        bool runs(int s, int t) const { const Frames r = range(s, t + 1); return r.t0 <= t && t < r.t1; }      // (t + 1: any bound above t stands for "all T")
        TailPlan plan{TailSchedule::Chains, false};      // what phase_b_start decided for this step (host/pipe_schedule.hpp)
        std::unique_ptr<std::atomic<int>[]> fgate; int fgate_n = 0;      // two chains / split rounds, per frame: depth stage done + previous flow stage done
        int retain_tag = -1;                                           // >= 0: the phase-A outputs of this step are kept under this tag when its tails are done
    } sb[2];
    // Phase-A outputs of a step kept beyond the step (sind_pipe_retain_next), so that sind_pipe_replay can run the stateful tails of those frames again from another state without
    // computing the state-free 99 % of the frame again (the repair runs of the chunked sequence mode).  Buffers come from a reserve made up front.
    struct Retained { PhaseAOut a; int tag = -1; };
    std::vector<std::unique_ptr<Retained>> spare, kept; int retain_tag_next = -1;
    int cur = 0; int occ_workers = 24;
    // CPU tokens (common.hpp) for the software-pipelined steps, where CalOccluded runners and tails compete for the quota (measured: throttled periods 7 -> 2
    // of 22, +1 %); synchronous steps run ungated -- there the hand-over of tokens at every GPU wait costs more than the throttling (tails 145 -> 173 ms)
    int cpu_tokens = 15, cpu_tokens_min = 13, cpu_tokens_max = 15;
    // Optional schedule of the synchronous step: run the depth half of the tails (k-means, SegAndMerge) underneath the dense flow.
    // Parity-tested, off by default: the tails phase shrinks from ~75 to ~23 ms, but the solver loses as much to the ~13 k extra small
    // launches it then shares the GPU with (dense flow 232 -> 287 ms at high stream priority; at normal priority the chains starve).
    bool depth_ahead = false;
    std::vector<char> primed;
    // Chunked sequences (sindslam_amd/sequence.py): hashing = every tail leaves the fingerprint of its rolled state per frame (last_hash: the step whose results
    // were returned last, [S][T][2]); active_next = per-stream number of frames whose TAILS run in the next step (one step only; empty = all T)
    std::vector<int> last_large_motion;      // large-motion flags of the step whose results were returned last, [S][T] (sind_pipe_large_motion)
    int last_schedule = -1;      // TailSchedule of that step (sind_pipe_last_schedule); -1: none yet
    bool hashing = false; std::vector<uint64_t> last_hash; std::vector<int> active_next; int chain_max_streams = 12; bool split_rounds = true;      /* rounds: the next k-means waits for the depth halves of the tails only (pipeline_rounds.cpp) */
    double stage_ms[6] = {0}; double tail_wait_ms = 0; double sor_ms = 0, sor_union_ms = 0, sor_bytes = 0; long long sor_launches = 0; int sor_slices = 1;      // launch groups of the large levels' solver in the last step (SorTimer kind 0: k_sor_wave by default, k_sor_stream with wave = 0)
    double sor_other_ms = 0, sor_other_bytes = 0; long long sor_other_launches = 0;                             // every other solver kernel outside k_coarse_chain (tiles, one-workgroup levels)
    SindHostGate gate;           // CPU tokens of this handle's pool tasks (common.hpp)
    WorkerPool workers;          // declared last: joined first
};

static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// One step of the grow-share controller (see sind_pipe::grow_q).  host_wait_ms: how long the step waited for host work after its GPU work was done;
// step_ms: wall time of the step.  The GPU is the scarcer resource of the two (a frame's grow costs one compute unit ~6 ms against one core ~5 ms, and a
// box has 256 of the one and 16 of the other -- but the solver wants all 256), so the share settles at the SMALLEST one the host keeps up with: a quarter
// more to the GPU as soon as a step waits for the host (> 3 % of the step), a quarter back after three steps in a row without any wait (< 0.5 %).
static inline void grow_adapt(sind_pipe* p, double host_wait_ms, double step_ms) {
    if (p->grow_q_fixed >= 0 || !p->batch_occ || step_ms <= 0) return;
    if (host_wait_ms > 0.03 * step_ms) {
        if ((p->grow_q >= 4 || host_wait_ms > 0.15 * step_ms) && p->batch_km && p->km_groups_fixed < 0) p->km_groups = std::min(p->km_groups_max, p->km_groups + 1);      // every grow is on the GPU already (or the wait is long): one more k-means chain
        p->grow_q = std::min(4, p->grow_q + 1); p->grow_idle_steps = 0;
        // clearly host-bound (the step waits for the tails for > 10 % of its time): a few more tokens than cores (a token is held through short waits too: 1280 x 720 + 3 - 6 %); else one more, up to share - 1
        p->cpu_tokens = host_wait_ms > 0.10 * step_ms ? p->cpu_tokens_max : std::max(p->cpu_tokens, std::min(p->cpu_tokens_max - 3, p->cpu_tokens + 1));
    } else if (host_wait_ms < 0.005 * step_ms) {
        p->cpu_tokens = std::max(p->cpu_tokens_min, p->cpu_tokens - 1);
        if (++p->grow_idle_steps >= 3) {
            if (p->batch_km && p->km_groups > 1 && p->km_groups_fixed < 0) p->km_groups--; else p->grow_q = std::max(0, p->grow_q - 1);
            p->grow_idle_steps = 0;
        }
    } else p->grow_idle_steps = 0;
}

// max filter of the 0/125/255 image with the 15x15 ellipse = two binary dilations (>=125, ==255)
static inline void dilate15_codes(const uint8_t* src, int W, int H, uint8_t* dst) {
    const EllipseElem e15(15);
    BitImg hi = BitImg::from_equal(src, W, H, W, 255), any = BitImg::from_u8(src, W, H, W);
    hi = hi.dilated(e15); any = any.dilated(e15);
    any.to_u8(dst, W, 125); hi.paint_u8(dst, W, 255);
}

// Tail / CalOccluded streams are high priority: their small kernels overtake the batch stream's flow solver when both are in flight.
// (A CU partition via hipExtStreamCreateWithCUMask was measured on MI355X: every masked stream ran 3-4x slower, see DESIGN.md.)
static inline int make_stream(hipStream_t* out, bool high_priority) {
    if (high_priority) { int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi); HIP_TRY(hipStreamCreateWithPriority(out, hipStreamNonBlocking, hi)); }
    else HIP_TRY(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    return SIND_OK;
}

// ---- the parts of the pipeline: pipeline_build.cpp (handle, streams, pool), pipeline_phase_a.cpp (the state-free batch of a step), phase B = pipeline_frame.cpp (what a frame's tail
// does), pipeline_chains.cpp, pipeline_rounds.cpp, pipeline_phase_b.cpp (schedule decision, start, finish), pipeline_capi.cpp (the C ABI: steps, state blobs, replay, settings, statistics)
struct PipeOut { uint8_t *dyna, *label, *mask; sind_keypoint* kps; int cap; int* nkp; uint8_t* desc; };
typedef sind_pipe::StepBuf StepBuf;
int pipe_build(sind_pipe* p, const sind_pipe_config* cfg);
int ensure_dtails(sind_pipe* p);
DynaTail* depth_half(sind_pipe* p, int s);
int phase_a(sind_pipe* p, StepBuf& sb, const uint8_t* bgr_dev, const uint16_t* depth_dev, double t[4], bool depth_ahead = false);
// (km / fm: the frame's share of a round's batched k-means and flow-mask stage, or null)
bool tail_one(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int worker, const KmFrameResult* km, const FlowMasksReady* fm = nullptr);
void tail_rag_begin(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int g, int worker, const KmFrameResult* km, const FlowMasksReady* fm);
void tail_pieces_begin(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int g, int worker, const KmFrameResult* km, const FlowMasksReady* fm);
void depth_task(sind_pipe* p, StepBuf* sb, int k, int worker);
void tail_task(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int worker);
void depth_chain(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t0, int t1, int worker);
void flow_chain(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int t1, int worker);
void arm_flow_gates(sind_pipe* p, StepBuf& sb);
void start_rounds(sind_pipe* p, StepBuf* sb, const PipeOut& o);
void phase_b_start(sind_pipe* p, StepBuf& sb, const PipeOut& o);
int phase_b_finish(sind_pipe* p, StepBuf& sb);
int phase_b(sind_pipe* p, StepBuf& sb, const PipeOut& o);
