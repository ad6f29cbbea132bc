// sind_pipe: phase B of a step -- the stateful tails on the worker pool (see pipeline_impl.hpp).
#include "pipeline_impl.hpp"

// ---- phase B of one step (stateful tails on the worker pool)
// One task = one frame of one stream; it queues the stream's next frame when it is done.  Frames of a stream stay in order, and the
// pool always sees up to S runnable tasks, so the workers stay busy until the end of the phase (a task per stream left the second
// "round" of 32 streams on 24 workers half empty).
// Depth half of frame k = (stream s, frame t) of a synchronous step: runs while the dense flow is on the GPU, in frame order per stream
// (the k-means warm labels are the previous frame's merged labels).  It opens the gate of the stream's next frame when it is done.
void depth_task(sind_pipe* p, sind_pipe::StepBuf* sb, int k, int worker) {
    for (;;) {
        const int T = p->T, s = k / T, t = k % T; const size_t np = (size_t)p->c.width * p->c.height;
        DynaTail* dt = depth_half(p, s); dt->stream = p->worker_streams_lo[worker];
        const int r = dt->depth_stage(sb->depth_h.data() + np * k, sb->depth_dev.p + np * k, &sb->occ[k], sb->dout[k]);
        if (r != SIND_OK) { sb->depth_rc[k] = r; sb->depth_err[k] = sind_last_error(); }
        if (!(t + 1 < T && sb->gate[k + 1].fetch_add(1) == 1)) return;
        if (p->S == 1) { k++; continue; }                    // one stream: the next frame's chain link right here (no hand-over to another worker)
        p->workers.push(sb->depth_group, [p, sb, k](int w) { depth_task(p, sb, k + 1, w); }); return;
    }
}
// what follows the fusion of a frame: state hash, dilation, the outputs, the keypoint filter (dy / lb: the frame's dynamic-area codes and labels)
static bool tail_finish(sind_pipe* p, sind_pipe::StepBuf* sb, PipeOut o, int s, int t, std::vector<uint8_t>& dy, std::vector<uint8_t>& lb) {
    const int T = p->T, W = p->c.width, H = p->c.height; const size_t np = (size_t)W * H;
    static thread_local std::vector<uint8_t> dil;
    dil.resize(np);
    const int k = s * T + t;
    if (p->hashing) { sb->state_hash[2 * (size_t)k] = p->tails[s]->state_hash[0]; sb->state_hash[2 * (size_t)k + 1] = p->tails[s]->state_hash[1]; }
    double* tf = p->tails[s]->t_fine; double t0 = now_ms();
    dilate15_codes(dy.data(), W, H, dil.data());
    { const double t1 = now_ms(); tf[30] += t1 - t0; t0 = t1; }
    if (o.dyna) std::memcpy(o.dyna + np * k, dy.data(), np);
    if (o.label) std::memcpy(o.label + np * k, lb.data(), np);
    if (o.mask) std::memcpy(o.mask + np * k, dil.data(), np);
    { const double t1 = now_ms(); tf[31] += t1 - t0; t0 = t1; }
    std::vector<OrbKeyPoint> kk; std::vector<uint8_t> dd;
    p->orb.finish(sb->orb[k], dil.data(), W, kk, dd);
    { const double t1 = now_ms(); tf[32] += t1 - t0; t0 = t1; }
    if ((int)kk.size() > o.cap && (o.kps || o.desc)) { sb->tail_rc[s] = SIND_E_CAPACITY; sb->tail_err[s] = "keypoint capacity exceeded"; return false; }
    if (o.nkp) o.nkp[k] = (int)kk.size();
    if (o.kps) std::memcpy(o.kps + (size_t)k * o.cap, kk.data(), kk.size() * sizeof(sind_keypoint));
    if (o.desc) std::memcpy(o.desc + (size_t)k * o.cap * 32, dd.data(), dd.size());
    return true;
}
static bool tail_one(sind_pipe* p, sind_pipe::StepBuf* sb, PipeOut o, int s, int t, int worker, const KmFrameResult* km, const FlowMasksReady* fm = nullptr) {
    SindRange range_t("sind tail: flow masks, SegAndMerge, fusion, dilation, ORB mask filter");
    p->tails[s]->stream = p->worker_streams[worker];
    const size_t np = (size_t)p->c.width * p->c.height;
    static thread_local std::vector<uint8_t> dy, lb;
    dy.resize(np); lb.resize(np);
    const int k = s * p->T + t;
    int r = (sb->depth_ahead || sb->two_chain) ? p->tails[s]->flow_stage(sb->U.p + np * k, sb->V.p + np * k, sb->dout[k], dy.data(), lb.data(), sb->occ[k].gridFlow, fm)
                            : p->tails[s]->process(sb->depth_h.data() + np * k, sb->depth_dev.p + np * k, sb->U.p + np * k, sb->V.p + np * k, dy.data(), lb.data(), &sb->occ[k],
                                                   p->dtails.empty() ? nullptr : (p->dtails[s]->stream = p->worker_streams[worker], p->dtails[s].get()), km, fm);
    if (r != SIND_OK) { sb->tail_rc[s] = r; sb->tail_err[s] = sind_last_error(); return false; }
    return tail_finish(p, sb, o, s, t, dy, lb);
}
// ---- a frame's tail in two tasks around the round's batched RAG stage (RagBatch, dyna.hpp; non-split rounds).  The first runs the frame up to SegAndMerge's pieces, takes
// a slot of the group's batch, packs its planes into the slab and joins.  Slots are handed out in the order the frames get there, a chunk is a run of slots: the frame
// that packs the last slot of a chunk -- or the last frame of the round, for the partial chunk at the end -- enqueues the chunk, waits once for its event and queues the
// second tasks of the chunk's frames (its own it runs itself).  A frame without pieces, or one the slab has no room for (it takes the per-frame stage), goes straight on.
static void tail_rag_end(sind_pipe* p, sind_pipe::StepBuf* sb, PipeOut o, int s, int t, int worker, const int* rag) {
    SindRange range_t("sind tail: SegAndMerge from the counters on, fusion, dilation, ORB mask filter");
    p->tails[s]->stream = p->worker_streams[worker]; if (!p->dtails.empty()) p->dtails[s]->stream = p->worker_streams[worker];
    const size_t np = (size_t)p->c.width * p->c.height;
    static thread_local std::vector<uint8_t> dy, lb;
    dy.resize(np); lb.resize(np);
    const int r = p->tails[s]->process_end(rag, dy.data(), lb.data());
    if (r != SIND_OK) { sb->tail_rc[s] = r; sb->tail_err[s] = sind_last_error(); return; }
    tail_finish(p, sb, o, s, t, dy, lb);
}
static void tail_rag_begin(sind_pipe* p, sind_pipe::StepBuf* sb, PipeOut o, int s, int t, int g, int worker, const KmFrameResult* km, const FlowMasksReady* fm) {
    RagBatch& rb = p->ragb[g]; sind_pipe::RagRound& rr = p->ragr[g];
    int slot = -1; const int* own = nullptr; int r;
    { SindRange range_t("sind tail: flow masks, SegAndMerge up to the packed planes");
      DynaTail* tl = p->tails[s].get(); tl->stream = p->worker_streams[worker];
      const size_t np = (size_t)p->c.width * p->c.height; const int k = s * p->T + t;
      r = tl->process_begin(sb->depth_h.data() + np * k, sb->depth_dev.p + np * k, sb->U.p + np * k, sb->V.p + np * k, &sb->occ[k],
                            p->dtails.empty() ? nullptr : (p->dtails[s]->stream = p->worker_streams[worker], p->dtails[s].get()), km, fm);
      DynaTail* h = tl->rag_half();
      if (r == SIND_OK && h->rag_pieces() > 0) {
          unsigned long long *pieces = nullptr, *conn = nullptr;
          if (h->rag_batchable() && rb.reserve(h->rag_pieces(), &slot, &pieces, &conn)) {
              const double tp = now_ms(); h->rag_pack(pieces, conn); h->t_fine[10] += now_ms() - tp; const OccResult* pre = h->rag_pre(); rb.set_inputs(slot, pre->occ2_dev, pre->depthN_dev, pre->occ2_event);
          } else { slot = -1; p->rag_fallback++; r = h->rag_own(&own); }
      }
      if (r != SIND_OK) { sb->tail_rc[s] = r; sb->tail_err[s] = sind_last_error(); } }
    int flush[2] = {-1, -1}, flush_n[2] = {0, 0}, nf = 0;      // (two when this frame fills its chunk and is also the round's last, behind frames of the partial chunk at the end)
    { std::lock_guard<std::mutex> lk(rr.m);
      if (slot >= 0) { rr.stream_of_slot[slot] = s; const int c = rb.chunk_of(slot); if (++rr.joined[c] == rb.chunk_frames()) { flush[nf] = c; flush_n[nf++] = rb.chunk_frames(); } }
      if (++rr.arrived == rr.expected && rb.slots() > 0) {                 // the last frame of the round: the partial chunk at the end, if there is one
          const int lc = rb.chunk_of(rb.slots() - 1), n = rb.chunk_count(lc);
          if (n < rb.chunk_frames()) { flush[nf] = lc; flush_n[nf++] = n; }
      } }
    bool mine = false;
    for (int f = 0; f < nf; f++) {
        const double te = now_ms();
        int rc = rb.enqueue(flush[f]); if (rc == SIND_OK) rc = rb.wait(flush[f]);
        p->tails[s]->t_fine[8] += now_ms() - te;      // (SIND_TAIL_TIMING's "rag": with the batch, the enqueuing frame's enqueue and wait for its whole chunk)
        const std::string e = rc == SIND_OK ? std::string() : "batched RAG statistics: " + std::string(sind_last_error());
        for (int b = rb.chunk_first(flush[f]); b < rb.chunk_first(flush[f]) + flush_n[f]; b++) {
            const int s2 = rr.stream_of_slot[b];
            if (rc != SIND_OK) { sb->tail_rc[s2] = rc; sb->tail_err[s2] = e; continue; }
            p->rag_frames++;
            if (s2 == s) { mine = true; continue; }
            const int* res = rb.result(b);
            p->workers.push(sb->km_tails[g], [p, sb, o, s2, t, res](int w) { tail_rag_end(p, sb, o, s2, t, w, res); });
        }
    }
    if (r != SIND_OK || sb->tail_rc[s] != SIND_OK) return;
    if (slot < 0) { if (!own) p->rag_frames++; tail_rag_end(p, sb, o, s, t, worker, own); }      // (no pieces: nothing to count, the frame did not leave the batched path)
    else if (mine) tail_rag_end(p, sb, o, s, t, worker, rb.result(slot));
}
static void tail_task(sind_pipe* p, sind_pipe::StepBuf* sb, PipeOut o, int s, int t, int worker, const KmFrameResult* km = nullptr, bool chain = true, const FlowMasksReady* fm = nullptr) {
    struct Spin { int keep; explicit Spin(bool on) : keep(t_sind_spin_us) { if (on) t_sind_spin_us = 400; } ~Spin() { t_sind_spin_us = keep; } } spin(sb->few_chain);      // few chains, idle host: poll before sleeping (common.hpp)
    for (;;) {
        if (!tail_one(p, sb, o, s, t, worker, km, fm) || !chain || t + 1 >= (sb->active.empty() ? p->T : std::min(p->T, sb->active[s]))) return;
        if (p->S == 1 || sb->few_chain) { t++; km = nullptr; fm = nullptr; continue; }      // one stream / a few chains: the next frame's chain link right here (no hand-over to another worker)
        p->workers.push(sb->tail_group, [p, sb, o, s, t](int w) { tail_task(p, sb, o, s, t + 1, w); }); return;
    }
}
// Two chains per stream for a handful of live streams (the slow runners of a repair): the depth chain -- k-means from the previous frame's merged labels, SegAndMerge; it
// needs nothing from the flow half -- runs ahead on the stream's depth-half object, the flow chain (flow masks, fusion, dilation, keypoint filter) follows frame by frame
// as soon as its frame's depth stage and the previous frame's flow stage are done.  A frame then costs max(depth, flow) instead of their sum (the in-order mode's schedule).
static void flow_chain(sind_pipe* p, sind_pipe::StepBuf* sb, PipeOut o, int s, int t, int t1, int worker, bool poll = true) {
    struct Spin { int keep; explicit Spin(bool on) : keep(t_sind_spin_us) { if (on) t_sind_spin_us = 400; } ~Spin() { t_sind_spin_us = keep; } } spin(poll);      // (a few chains on an idle host poll before they sleep; the rounds of a full pipeline do not)
    for (;;) {
        if (!tail_one(p, sb, o, s, t, worker, nullptr) || t + 1 >= t1) return;
        if (sb->fgate[s * p->T + t + 1].fetch_add(1) != 1) return;          // the next frame's depth stage is still out: its completion starts the flow stage
        t++;
    }
}
static void depth_chain(sind_pipe* p, sind_pipe::StepBuf* sb, PipeOut o, int s, int t0, int t1, int worker) {
    struct Spin { int keep; Spin() : keep(t_sind_spin_us) { t_sind_spin_us = 400; } ~Spin() { t_sind_spin_us = keep; } } spin;
    const size_t np = (size_t)p->c.width * p->c.height;
    DynaTail* dt = p->dtails[s].get(); dt->stream = p->worker_streams_lo[worker];
    for (int t = t0; t < t1; t++) {
        const int k = s * p->T + t;
        const int r = dt->depth_stage(sb->depth_h.data() + np * k, sb->depth_dev.p + np * k, &sb->occ[k], sb->dout[k], nullptr);
        if (r != SIND_OK) { sb->dchain_rc[s] = r; sb->dchain_err[s] = sind_last_error(); return; }      // the flow chain of this stream stops at the frame before
        if (sb->fgate[k].fetch_add(1) == 1) p->workers.push(sb->tail_group, [p, sb, o, s, t, t1](int w) { flow_chain(p, sb, o, s, t, t1, w); });
    }
}
// a round's batched flow-mask stage as its round thread sees it: the slot of every stream of the group in the batch (-1: no frame in this round), the homography
// tasks still out, the first failure, and the masks handed to the tails
struct FmRound {
    std::vector<int> slot; std::vector<FlowMasksReady> ready; int n = 0; std::atomic<int> left{0};
    std::mutex m; int rc = SIND_OK; std::string err;
    void fail(int r, const std::string& e) { std::lock_guard<std::mutex> lk(m); if (rc == SIND_OK) { rc = r; err = e; } }
};
void phase_b_start(sind_pipe* p, sind_pipe::StepBuf& sb, const PipeOut& o) {
    const int S = p->S;
    sb.tail_rc.assign(S, SIND_OK); sb.tail_err.assign(S, std::string()); sb.dchain_rc.assign(S, SIND_OK); sb.dchain_err.assign(S, std::string());
    sind_pipe::StepBuf* sbp = &sb;
    // A step in which only a few streams have frames (the repair runs of the chunked sequence mode: the slow runners of a round, sind_pipe_replay) runs them as
    // per-stream chains with their own k-means launches instead of rounds: a round costs the batched k-means' ~60 dependent launches for every frame whatever the
    // batch, and its barrier makes every stream wait for the slowest tail -- with a handful of streams on an otherwise idle GPU the chains are about twice as fast.
    int nact = 0; for (int s = 0; s < S; s++) nact += (sb.first.empty() ? 0 : sb.first[s]) < (sb.active.empty() ? p->T : sb.active[s]);
    const bool few = (!sb.first.empty() || !sb.active.empty()) && nact <= p->chain_max_streams;
    sb.few_chain = few && S > 1; sb.two_chain = false;
    if (sb.few_chain && !sb.depth_ahead && ensure_dtails(p) == SIND_OK) {
        const int B = S * p->T;
        if (sb.fgate_n < B) { sb.fgate.reset(new std::atomic<int>[B]); sb.fgate_n = B; }
        sb.dout.assign(B, DepthStageOut()); sb.two_chain = true;
        for (int s = 0; s < S; s++) {
            const int t0 = sb.first.empty() ? 0 : sb.first[s], t1 = sb.active.empty() ? p->T : sb.active[s];
            if (t0 >= t1) continue;
            for (int t = t0; t < t1; t++) sb.fgate[s * p->T + t].store(t == t0 ? 1 : 0);
            p->workers.push(sb.tail_group, [p, sbp, o, s, t0, t1](int w) { depth_chain(p, sbp, o, s, t0, t1, w); });
        }
        return;
    }
    if (p->batch_km && !sb.depth_ahead && !few) {
        // rounds: frame t of every stream -- the batched k-means chain on its own stream, then the S tails of that frame on the pool.
        // split (default): what the NEXT round's k-means waits for is only the depth half of a tail (cluster order, SegAndMerge: its merged labels start that k-means); the flow
        // half (flow masks, fusion, dilation, keypoint filter) of frame t follows on the stream's tail object as soon as its depth half and the flow half of frame t - 1 are
        // done, beside the next round.  A chunk's frames are a serial chain: this takes ~a third of a frame's tail off it.
        // Measured (profiles/r05/ab_split_rounds.txt): 5 streams x 6 frames 562 - 582 -> 665 - 676 pairs/s, 8 x 4 745 - 758 -> 816 - 826, 16 x 2 and 32 x 2 unchanged, 128 x 4 within
        // noise on the losing side -- so only while there are no more streams than pool workers (with more, other streams' tails fill the pool during a round anyway).
        const bool split = p->split_rounds && S <= (int)p->worker_streams.size() && ensure_dtails(p) == SIND_OK;
        if (split) {
            const int B = S * p->T;
            if (sb.fgate_n < B) { sb.fgate.reset(new std::atomic<int>[B]); sb.fgate_n = B; }
            sb.dout.assign(B, DepthStageOut()); sb.two_chain = true;
            for (int s = 0; s < S; s++) { const int t0 = sb.first.empty() ? 0 : sb.first[s]; for (int t = 0; t < p->T; t++) sb.fgate[s * p->T + t].store(t == t0 ? 1 : 0); }
        }
        sbp->km_groups = p->km_groups; for (int g = 0; g <= sbp->km_groups; g++) sbp->km_first[g] = (int)((long long)S * g / sbp->km_groups);
        for (int g = 0; g < sbp->km_groups; g++) p->round_threads.emplace_back([p, sbp, o, g, split] {
            (void)pthread_setname_np(pthread_self(), "sind-rounds"); (void)hipSetDevice(p->c.device);
            const size_t np = (size_t)p->c.width * p->c.height;
            const int s0 = sbp->km_first[g], ns = sbp->km_first[g + 1] - s0; std::vector<const uint8_t*> prev(ns);
            FmRound fm; fm.slot.assign(ns, -1); fm.ready.resize(ns);
            for (int t = 0; t < p->T; t++) {
                bool any = false;                                        // ragged / replayed steps: rounds in which no stream of the group has a frame are passed over
                for (int s = s0; s < s0 + ns && !any; s++) any = (sbp->first.empty() || t >= sbp->first[s]) && (sbp->active.empty() || t < sbp->active[s]);
                if (!any) continue;
                if (t > 0) WorkerPool::wait(sbp->km_tails[g]);           // this group's tails (split: their depth halves) of frame t - 1: their merged labels start this round's k-means
                for (int s = 0; s < ns; s++) prev[s] = depth_half(p, s0 + s)->prev_km_labels();
                // Batched flow-mask stage of this round (non-split rounds only: with split rounds the flow half of frame t - 1 may still be running here, and its state is
                // what the homography starts from).  One homography task per stream with a frame in this round; whichever finishes last enqueues the group's launches.
                fm.n = 0; fm.rc = SIND_OK;
                if (p->fm_batch && !split) for (int s = s0; s < s0 + ns; s++)
                    if (sbp->tail_rc[s] == SIND_OK && (sbp->first.empty() || t >= sbp->first[s]) && (sbp->active.empty() || t < sbp->active[s])) fm.slot[s - s0] = fm.n++; else fm.slot[s - s0] = -1;
                if (fm.n > 0) {
                    fm.left.store(fm.n);
                    FmRound* f = &fm;
                    for (int s = s0; s < s0 + ns; s++) if (fm.slot[s - s0] >= 0) p->workers.push(sbp->fm_group[g], [p, sbp, f, s, t, g, s0, np](int w) {
                        const int k = s * p->T + t; double Hm[9];
                        DynaTail* tl = p->tails[s].get(); tl->stream = p->worker_streams[w];
                        int r = tl->flow_masks_homography(sbp->U.p + np * k, sbp->V.p + np * k, sbp->occ[k].gridFlow, Hm);
                        if (r == SIND_OK) r = p->fmb[g].set(f->slot[s - s0], tl, sbp->U.p + np * k, sbp->V.p + np * k, Hm);
                        if (r != SIND_OK) f->fail(r, sind_last_error());
                        if (f->left.fetch_sub(1) != 1) return;
                        if (f->rc == SIND_OK && (r = p->fmb[g].enqueue(f->n)) != SIND_OK) f->fail(r, sind_last_error());
                    });
                }
                const double tk = now_ms();
                int rc;
                { SindRange range_km("sind round: batched k-means of frame t of one group of streams");
                  rc = p->kmb[g].run(sbp->depth_dev.p + np * ((size_t)s0 * p->T + t), np * p->T, ns, prev.data()); }
                { std::lock_guard<std::mutex> lk(p->km_stat_mu); p->km_round_ms += now_ms() - tk; p->km_rounds++; }
                if (fm.n > 0) {              // (also when the k-means failed: the tasks point at this thread's round state)
                    WorkerPool::wait(sbp->fm_group[g]);
                    if (fm.rc == SIND_OK) { const int r = p->fmb[g].wait(); if (r != SIND_OK) fm.fail(r, sind_last_error()); }
                    if (fm.rc == SIND_OK) { for (int s = 0; s < ns; s++) if (fm.slot[s] >= 0) fm.ready[s] = p->fmb[g].result(fm.slot[s]); p->fm_frames += fm.n; }
                }
                if (rc != SIND_OK) { const std::string e = sind_last_error(); for (int s = s0; s < s0 + ns; s++) if (sbp->tail_rc[s] == SIND_OK) { sbp->tail_rc[s] = rc; sbp->tail_err[s] = "batched k-means: " + e; } return; }
                if (fm.rc != SIND_OK) { for (int s = s0; s < s0 + ns; s++) if (sbp->tail_rc[s] == SIND_OK) { sbp->tail_rc[s] = fm.rc; sbp->tail_err[s] = "batched flow masks: " + fm.err; } return; }
                // batched RAG stage of this round (non-split rounds only, like the flow masks'): the round's frames are counted before the first of them is queued
                const bool ragb = p->rag_batch && !split;
                if (ragb) {
                    sind_pipe::RagRound& rr = p->ragr[g]; int n = 0;
                    for (int s = s0; s < s0 + ns; s++) n += sbp->tail_rc[s] == SIND_OK && (sbp->first.empty() || t >= sbp->first[s]) && (sbp->active.empty() || t < sbp->active[s]);
                    p->ragb[g].set_limits(p->rag_chunk, p->rag_planes);
                    const int r = p->ragb[g].begin_round();
                    if (r != SIND_OK) { const std::string e = sind_last_error(); for (int s = s0; s < s0 + ns; s++) if (sbp->tail_rc[s] == SIND_OK) { sbp->tail_rc[s] = r; sbp->tail_err[s] = "batched RAG statistics: " + e; } return; }
                    std::lock_guard<std::mutex> lk(rr.m); rr.expected = n; rr.arrived = 0; rr.joined.assign(ns + 1, 0); rr.stream_of_slot.assign(ns, -1);
                }
                for (int s = s0; s < s0 + ns; s++) {
                    if (!(sbp->tail_rc[s] == SIND_OK && (sbp->first.empty() || t >= sbp->first[s]) && (sbp->active.empty() || t < sbp->active[s]))) continue;
                    if (ragb) { const bool have = fm.n > 0; const FlowMasksReady fr = have ? fm.ready[s - s0] : FlowMasksReady{nullptr, nullptr, nullptr};
                                p->workers.push(sbp->km_tails[g], [p, sbp, o, s, t, g, s0, fr, have](int w) { tail_rag_begin(p, sbp, o, s, t, g, w, &p->kmb[g].result(s - s0), have ? &fr : nullptr); }); continue; }
                    if (!split) { const bool have = fm.n > 0; const FlowMasksReady fr = have ? fm.ready[s - s0] : FlowMasksReady{nullptr, nullptr, nullptr};      // (by value: this thread may be gone when the task runs; the masks themselves stay until the group's next enqueue)
                                  p->workers.push(sbp->km_tails[g], [p, sbp, o, s, t, g, s0, fr, have](int w) { tail_task(p, sbp, o, s, t, w, &p->kmb[g].result(s - s0), false, have ? &fr : nullptr); }); continue; }
                    p->workers.push(sbp->km_tails[g], [p, sbp, o, s, t, g, s0, np](int w) {
                        const int k = s * p->T + t, t1 = sbp->active.empty() ? p->T : std::min(p->T, sbp->active[s]);
                        DynaTail* dt = p->dtails[s].get(); dt->stream = p->worker_streams[w];      // (on the chain that the next round waits for: the pool's high-priority stream)
                        const int r = dt->depth_stage(sbp->depth_h.data() + np * k, sbp->depth_dev.p + np * k, &sbp->occ[k], sbp->dout[k], &p->kmb[g].result(s - s0));
                        if (r != SIND_OK) { sbp->dchain_rc[s] = r; sbp->dchain_err[s] = sind_last_error(); return; }      // the flow halves of this stream stop at the frame before
                        if (sbp->fgate[k].fetch_add(1) == 1) p->workers.push(sbp->tail_group, [p, sbp, o, s, t, t1](int w2) { flow_chain(p, sbp, o, s, t, t1, w2, false); });
                    });
                }
            } });
        return;
    }
    for (int s = 0; s < S; s++) {
        const int t0 = sb.first.empty() ? 0 : sb.first[s], t1 = sb.active.empty() ? p->T : sb.active[s];
        if (t0 < t1) p->workers.push(sb.tail_group, [p, sbp, o, s, t0](int w) { tail_task(p, sbp, o, s, t0, w); });
    }
}
void swap_phase_a_outputs(sind_pipe::StepBuf& sb, sind_pipe::Retained& r) {
    sb.U.swap(r.U); sb.V.swap(r.V); sb.grid_dev.swap(r.grid_dev); sb.depth_dev.swap(r.depth_dev); sb.depth_h.swap(r.depth_h); sb.grid_h.swap(r.grid_h);
    sb.occ2_dev.swap(r.occ2_dev); sb.depthN_dev.swap(r.depthN_dev); sb.orb.swap(r.orb); sb.occ.swap(r.occ); sb.large_motion.swap(r.large_motion);
}
int phase_b_finish(sind_pipe* p, sind_pipe::StepBuf& sb) {
    for (std::thread& t : p->round_threads) if (t.joinable()) t.join();
    p->round_threads.clear();
    for (TaskGroup& g : sb.km_tails) WorkerPool::wait(g);      // (first: with split rounds a depth half queues its frame's flow half into tail_group when it is done)
    WorkerPool::wait(sb.tail_group);
    sb.pending = false;
    p->last_hash = sb.state_hash; p->last_large_motion = sb.large_motion;
    if (sb.retain_tag >= 0) {                       // keep this step's phase-A outputs: they change places with a reserve set of the same sizes
        if (p->spare.empty()) { sind_set_error("sind_pipe: no reserve left to retain step %d (sind_pipe_reserve_retained)", sb.retain_tag); sb.retain_tag = -1; return SIND_E_STATE; }
        std::unique_ptr<sind_pipe::Retained> r = std::move(p->spare.back()); p->spare.pop_back();
        swap_phase_a_outputs(sb, *r); r->tag = sb.retain_tag; sb.retain_tag = -1;
        for (OccResult& o : r->occ) o.occ2_event = nullptr;            // the uploads behind these events are long done; the events belong to the step buffer and are recorded again
        p->kept.push_back(std::move(r));
    }
    for (int s = 0; s < p->S; s++) if (sb.tail_rc[s] != SIND_OK) { sind_set_error("stream %d: %s", s, sb.tail_err[s].c_str()); return sb.tail_rc[s]; }
    for (int s = 0; s < p->S && s < (int)sb.dchain_rc.size(); s++) if (sb.dchain_rc[s] != SIND_OK) { sind_set_error("stream %d (depth chain): %s", s, sb.dchain_err[s].c_str()); return sb.dchain_rc[s]; }
    return SIND_OK;
}
int phase_b(sind_pipe* p, sind_pipe::StepBuf& sb, const PipeOut& o) { phase_b_start(p, sb, o); return phase_b_finish(p, sb); }

