// sind_pipe, phase B: frame t of a group of streams as a round (see pipeline_impl.hpp; host/pipe_schedule.hpp says when).
// Rounds: the batched k-means chain on the group's own stream, the flow-mask and RAG stages batched beside and behind it, then the tails of that frame on the pool.
// Split rounds: what the NEXT round's k-means waits for is only the depth half of a tail (cluster order, SegAndMerge: its merged labels start that k-means); the flow
// half (flow masks, fusion, dilation, keypoint filter) of frame t follows on the stream's tail object as soon as its depth half and the flow half of frame t - 1 are
// done, beside the next round.  A chunk's frames are a serial chain: this takes ~a third of a frame's tail off it.  The batched flow-mask and RAG stages are for the
// non-split rounds only: with split rounds the flow half of frame t - 1 may still be running when round t starts, and its state is what the homography starts from.
// Measured (profiles/r05/ab_split_rounds.txt): 5 streams x 6 frames 562 - 582 -> 665 - 676 pairs/s, 8 x 4 745 - 758 -> 816 - 826, 16 x 2 and 32 x 2 unchanged, 128 x 4 within
// noise on the losing side.
#include "pipeline_impl.hpp"

// a round's batched flow-mask stage as its round thread sees it: the slot of every stream of the group in the batch (-1: no frame in this round), the homography
// tasks still out, the first failure, and the masks handed to the tails
struct FmRound {
    std::vector<int> slot; std::vector<FlowMasksReady> ready; int n = 0; std::atomic<int> left{0};
    std::mutex m; Failures first;
    void fail(int r) { const std::string e = sind_last_error(); std::lock_guard<std::mutex> lk(m); if (first.ok(0)) first.fail(0, r, e); }
};
// one group's round thread: streams [s0, s0 + ns) of the step, round t
struct Round {
    sind_pipe* p; StepBuf* sb; PipeOut o; int g, s0, ns; bool split; size_t np; int t = 0;
    FmRound fm; std::vector<const uint8_t*> prev;
    bool live(int s) const { return sb->tail_fail.ok(s) && sb->runs(s, t); }      // stream s has a frame in this round and has not failed
};

// 1. the round's batched flow-mask stage: one homography task per live stream; whichever finishes last enqueues the group's launches
static void fm_begin(Round& r) {
    sind_pipe* p = r.p; StepBuf* sb = r.sb; FmRound* f = &r.fm; const int g = r.g, s0 = r.s0, t = r.t; const size_t np = r.np;
    f->n = 0; f->first.reset(1);
    if (p->fm_batch && !r.split) for (int s = s0; s < s0 + r.ns; s++) f->slot[s - s0] = r.live(s) ? f->n++ : -1;
    if (f->n == 0) return;
    f->left.store(f->n);
    for (int s = s0; s < s0 + r.ns; s++) if (f->slot[s - s0] >= 0) p->workers.push(sb->fm_group[g], [p, sb, f, s, t, g, s0, np](int w) {
        const int k = s * p->T + t; double Hm[9];
        DynaTail* tl = p->tails[s].get(); tl->stream = p->worker_streams[w];
        int rc = tl->flow_masks_homography(sb->a.U.p + np * k, sb->a.V.p + np * k, sb->a.occ[k].gridFlow, Hm);
        if (rc == SIND_OK) rc = p->fmb[g].set(f->slot[s - s0], tl, sb->a.U.p + np * k, sb->a.V.p + np * k, Hm);
        if (rc != SIND_OK) f->fail(rc);
        if (f->left.fetch_sub(1) != 1) return;
        if (f->first.ok(0) && (rc = p->fmb[g].enqueue(f->n)) != SIND_OK) f->fail(rc);
    });
}
// 2. the batched k-means of frame t, from the merged labels the previous round's tails (split: their depth halves) left
static int round_kmeans(Round& r) {
    sind_pipe* p = r.p; const double tk = now_ms(); int rc;
    { SindRange range_km("sind round: batched k-means of frame t of one group of streams");
      rc = p->kmb[r.g].run(r.sb->a.depth_dev.p + r.np * ((size_t)r.s0 * p->T + r.t), r.np * p->T, r.ns, r.prev.data()); }
    { std::lock_guard<std::mutex> lk(p->km_stat_mu); p->km_round_ms += now_ms() - tk; p->km_rounds++; }
    return rc;
}
// (the homography tasks point at this thread's round state: they are waited for also when the k-means failed)
static void fm_finish(Round& r) {
    FmRound& fm = r.fm; FlowMaskBatch& b = r.p->fmb[r.g];
    if (fm.n == 0) return;
    WorkerPool::wait(r.sb->fm_group[r.g]);
    if (fm.first.ok(0)) { const int rc = b.wait(); if (rc != SIND_OK) fm.fail(rc); }
    if (fm.first.ok(0)) { for (int s = 0; s < r.ns; s++) if (fm.slot[s] >= 0) fm.ready[s] = b.result(fm.slot[s]); r.p->fm_frames += fm.n; }
}
// 3. the round's batched RAG stage: the round's frames are counted before the first of them is queued
static int rag_open(Round& r) {
    sind_pipe* p = r.p; sind_pipe::RagRound& rr = p->ragr[r.g]; int n = 0;
    for (int s = r.s0; s < r.s0 + r.ns; s++) n += r.live(s);
    p->ragb[r.g].set_limits(p->rag_chunk, p->rag_planes);
    int rc = p->ragb[r.g].begin_round();
    if (rc == SIND_OK && p->pieces_batch) { p->pieceb[r.g].set_chunk(p->rag_chunk); rc = p->pieceb[r.g].begin_round(); }      // (the workspaces come with the first round that wants them)
    if (rc != SIND_OK) return rc;
    std::lock_guard<std::mutex> lk(rr.m); rr.expected = n; rr.arrived = 0; rr.joined.assign(r.ns + 1, 0); rr.stream_of_slot.assign(r.ns, -1);
    return SIND_OK;
}
// 4. the tails of the round's frames on the pool (everything by value: this thread may be gone when a task runs; the masks themselves stay until the group's next enqueue)
static void push_tails(Round& r, bool ragb) {
    sind_pipe* p = r.p; StepBuf* sb = r.sb; const PipeOut o = r.o; const int g = r.g, s0 = r.s0, t = r.t; const size_t np = r.np; const bool have = r.fm.n > 0;
    for (int s = s0; s < s0 + r.ns; s++) {
        if (!r.live(s)) continue;
        const FlowMasksReady fr = have ? r.fm.ready[s - s0] : FlowMasksReady{nullptr, nullptr, nullptr};
        if (ragb && p->pieces_batch) p->workers.push(sb->km_tails[g], [p, sb, o, s, t, g, s0, fr, have](int w) { tail_pieces_begin(p, sb, o, s, t, g, w, &p->kmb[g].result(s - s0), have ? &fr : nullptr); });
        else if (ragb) p->workers.push(sb->km_tails[g], [p, sb, o, s, t, g, s0, fr, have](int w) { tail_rag_begin(p, sb, o, s, t, g, w, &p->kmb[g].result(s - s0), have ? &fr : nullptr); });
        else if (!r.split) p->workers.push(sb->km_tails[g], [p, sb, o, s, t, g, s0, fr, have](int w) { tail_one(p, sb, o, s, t, w, &p->kmb[g].result(s - s0), have ? &fr : nullptr); });
        else p->workers.push(sb->km_tails[g], [p, sb, o, s, t, g, s0, np](int w) {
            const int k = s * p->T + t, t1 = sb->range(s, p->T).t1;
            DynaTail* dt = p->dtails[s].get(); dt->stream = p->worker_streams[w];      // (on the chain that the next round waits for: the pool's high-priority stream)
            const int rc = dt->depth_stage(sb->a.depth_h.data() + np * k, sb->a.depth_dev.p + np * k, &sb->a.occ[k], sb->dout[k], &p->kmb[g].result(s - s0));
            if (rc != SIND_OK) { sb->dchain_fail.fail(s, rc); return; }      // the flow halves of this stream stop at the frame before
            if (sb->fgate[k].fetch_add(1) == 1) p->workers.push(sb->tail_group, [p, sb, o, s, t, t1](int w2) { flow_chain(p, sb, o, s, t, t1, w2); });
        });
    }
}
static void round_thread(sind_pipe* p, StepBuf* sb, PipeOut o, int g) {
    (void)pthread_setname_np(pthread_self(), "sind-rounds"); (void)hipSetDevice(p->c.device);
    Round r{p, sb, o, g, sb->km_first[g], sb->km_first[g + 1] - sb->km_first[g], sb->plan.kind == TailSchedule::SplitRounds, p->np()};
    r.prev.resize(r.ns); r.fm.slot.assign(r.ns, -1); r.fm.ready.resize(r.ns);
    Failures& tf = sb->tail_fail; const int s1 = r.s0 + r.ns;
    for (r.t = 0; r.t < p->T; r.t++) {
        bool any = false;                                        // ragged / replayed steps: rounds in which no stream of the group has a frame are passed over
        for (int s = r.s0; s < s1 && !any; s++) any = sb->runs(s, r.t);
        if (!any) continue;
        if (r.t > 0) WorkerPool::wait(sb->km_tails[g]);          // this group's tails (split: their depth halves) of frame t - 1: their merged labels start this round's k-means
        for (int s = 0; s < r.ns; s++) r.prev[s] = depth_half(p, r.s0 + s)->prev_km_labels();
        fm_begin(r);
        const int rc = round_kmeans(r);
        fm_finish(r);
        if (rc != SIND_OK) { tf.fail_all(r.s0, s1, rc, "batched k-means: "); return; }
        if (!r.fm.first.ok(0)) { tf.fail_all(r.s0, s1, r.fm.first.rc[0], "batched flow masks: ", r.fm.first.err[0]); return; }
        const bool ragb = p->rag_batch && !r.split;
        if (ragb) { const int rr = rag_open(r); if (rr != SIND_OK) { tf.fail_all(r.s0, s1, rr, "batched RAG statistics: "); return; } }
        push_tails(r, ragb);
    }
}
void start_rounds(sind_pipe* p, StepBuf* sb, const PipeOut& o) {
    sb->km_groups = p->km_groups; for (int g = 0; g <= sb->km_groups; g++) sb->km_first[g] = (int)((long long)p->S * g / sb->km_groups);
    for (int g = 0; g < sb->km_groups; g++) p->round_threads.emplace_back(round_thread, p, sb, o, g);
}
