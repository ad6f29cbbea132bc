// sind_pipe, phase B: what the tail of one frame does, whatever schedule it is part of (see pipeline_impl.hpp).
#include "pipeline_impl.hpp"

// what follows the fusion of a frame: state hash, dilation, the outputs, the keypoint filter (dy / lb: the frame's dynamic-area codes and labels)
static bool tail_finish(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, std::vector<uint8_t>& dy, std::vector<uint8_t>& lb) {
    const int T = p->T, W = p->c.width, H = p->c.height; const size_t np = (size_t)W * H;
    static thread_local std::vector<uint8_t> dil;
    dil.resize(np);
    const int k = s * T + t;
    if (p->hashing) { sb->state_hash[2 * (size_t)k] = p->tails[s]->state_hash[0]; sb->state_hash[2 * (size_t)k + 1] = p->tails[s]->state_hash[1]; }
    double* tf = p->tails[s]->t_fine; double t0 = now_ms(); auto lap = [&](int i) { const double t1 = now_ms(); tf[i] += t1 - t0; t0 = t1; };
    dilate15_codes(dy.data(), W, H, dil.data());
    lap(30);
    if (o.dyna) std::memcpy(o.dyna + np * k, dy.data(), np);
    if (o.label) std::memcpy(o.label + np * k, lb.data(), np);
    if (o.mask) std::memcpy(o.mask + np * k, dil.data(), np);
    lap(31);
    std::vector<OrbKeyPoint> kk; std::vector<uint8_t> dd;
    p->orb.finish(sb->a.orb[k], dil.data(), W, kk, dd);
    lap(32);
    if ((int)kk.size() > o.cap && (o.kps || o.desc)) { sb->tail_fail.fail(s, SIND_E_CAPACITY, "keypoint capacity exceeded"); return false; }
    if (o.nkp) o.nkp[k] = (int)kk.size();
    if (o.kps) std::memcpy(o.kps + (size_t)k * o.cap, kk.data(), kk.size() * sizeof(sind_keypoint));
    if (o.desc) std::memcpy(o.desc + (size_t)k * o.cap * 32, dd.data(), dd.size());
    return true;
}
// the stream's tail and depth-half objects work on this worker's HIP stream for the length of a task
static DynaTail* on_worker(sind_pipe* p, int s, int worker) {
    p->tails[s]->stream = p->worker_streams[worker]; if (!p->dtails.empty()) p->dtails[s]->stream = p->worker_streams[worker];
    return p->dtails.empty() ? nullptr : p->dtails[s].get();
}
// a whole tail, or its flow half where the step's schedule ran the frame's depth stage ahead (sb->plan)
bool tail_one(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int worker, const KmFrameResult* km, const FlowMasksReady* fm) {
    SindRange range_t("sind tail: flow masks, SegAndMerge, fusion, dilation, ORB mask filter");
    PhaseAOut& a = sb->a; const size_t np = p->np();
    static thread_local std::vector<uint8_t> dy, lb;
    dy.resize(np); lb.resize(np);
    const int k = s * p->T + t; int r;
    if (runs_flow_halves(sb->plan.kind)) { p->tails[s]->stream = p->worker_streams[worker]; r = p->tails[s]->flow_stage(a.U.p + np * k, a.V.p + np * k, sb->dout[k], dy.data(), lb.data(), a.occ[k].gridFlow, fm); }
    else { DynaTail* dh = on_worker(p, s, worker); r = p->tails[s]->process(a.depth_h.data() + np * k, a.depth_dev.p + np * k, a.U.p + np * k, a.V.p + np * k, dy.data(), lb.data(), &a.occ[k], dh, km, fm); }
    if (r != SIND_OK) { sb->tail_fail.fail(s, r); return false; }
    return tail_finish(p, sb, o, s, t, dy, lb);
}
// ---- a frame's tail in two tasks around the round's batched RAG stage (RagBatch, dyna.hpp; non-split rounds).  The first runs the frame up to SegAndMerge's pieces, takes
// a slot of the group's batch, packs its planes into the slab and joins.  Slots are handed out in the order the frames get there, a chunk is a run of slots: the frame
// that packs the last slot of a chunk -- or the last frame of the round, for the partial chunk at the end -- enqueues the chunk, waits once for its event and queues the
// second tasks of the chunk's frames (its own it runs itself).  A frame without pieces, or one the slab has no room for (it takes the per-frame stage), goes straight on.
static void tail_rag_end(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int worker, const int* rag) {
    SindRange range_t("sind tail: SegAndMerge from the counters on, fusion, dilation, ORB mask filter");
    on_worker(p, s, worker);
    const size_t np = p->np();
    static thread_local std::vector<uint8_t> dy, lb;
    dy.resize(np); lb.resize(np);
    const int r = p->tails[s]->process_end(rag, dy.data(), lb.data());
    if (r != SIND_OK) { sb->tail_fail.fail(s, r); return; }
    tail_finish(p, sb, o, s, t, dy, lb);
}
// up to the packed planes: the frame's slot in the group's batch (-1: none), or *own = the counters of the per-frame stage it took instead
static int rag_pack_frame(sind_pipe* p, StepBuf* sb, int s, int t, int g, int worker, const KmFrameResult* km, const FlowMasksReady* fm, int* slot, const int** own) {
    SindRange range_t("sind tail: flow masks, SegAndMerge up to the packed planes");
    RagBatch& rb = p->ragb[g]; PhaseAOut& a = sb->a; DynaTail* tl = p->tails[s].get(); DynaTail* dh = on_worker(p, s, worker);
    const size_t np = p->np(); const int k = s * p->T + t;
    int r = tl->process_begin(a.depth_h.data() + np * k, a.depth_dev.p + np * k, a.U.p + np * k, a.V.p + np * k, &a.occ[k], dh, km, fm);
    DynaTail* h = tl->rag_half();
    if (r == SIND_OK && h->rag_pieces() > 0) {
        unsigned long long *pieces = nullptr, *conn = nullptr;
        if (h->rag_batchable() && rb.reserve(h->rag_pieces(), slot, &pieces, &conn)) {
            const double tp = now_ms(); h->rag_pack(pieces, conn); h->t_fine[10] += now_ms() - tp; const OccResult* pre = h->rag_pre(); rb.set_inputs(*slot, pre->occ2_dev, pre->depthN_dev, pre->occ2_event);
        } else { *slot = -1; p->rag_fallback++; r = h->rag_own(own); }
    }
    if (r != SIND_OK) sb->tail_fail.fail(s, r);
    return r;
}
void tail_rag_begin(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int g, int worker, const KmFrameResult* km, const FlowMasksReady* fm) {
    RagBatch& rb = p->ragb[g]; sind_pipe::RagRound& rr = p->ragr[g];
    int slot = -1; const int* own = nullptr;
    const int r = rag_pack_frame(p, sb, s, t, g, worker, km, fm, &slot, &own);
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
            if (rc != SIND_OK) { sb->tail_fail.fail(s2, rc, e); continue; }
            p->rag_frames++;
            if (s2 == s) { mine = true; continue; }
            const int* res = rb.result(b);
            p->workers.push(sb->km_tails[g], [p, sb, o, s2, t, res](int w) { tail_rag_end(p, sb, o, s2, t, w, res); });
        }
    }
    if (r != SIND_OK || !sb->tail_fail.ok(s)) return;
    if (slot < 0) { if (!own) p->rag_frames++; tail_rag_end(p, sb, o, s, t, worker, own); }      // (no pieces: nothing to count, the frame did not leave the batched path)
    else if (mine) tail_rag_end(p, sb, o, s, t, worker, rb.result(slot));
}
// ---- the same with the round's batched piece stage in front of the join (PieceBatch, dyna.hpp; sind_pipe_set_pieces_batch).  The first task runs the frame up to the INPUTS of
// the piece extraction, takes a slot of the group's piece batch, packs and joins; chunks and the round's last frame are found as above, on piece slots.  The frame that
// completes a chunk flushes it (piece_chunk_flush: piece launches, wait, the host step of every frame, the run of RAG slots, commit and paint launches, RAG launches,
// wait) and queues the other frames' second tasks: two waits per chunk, none per frame.  A frame the stage cannot take (no cluster to cut, inputs not on the device) runs
// the host function and the per-frame RAG stage in its own task, as it does without the switch.
static void tail_pieces_end(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int worker, const int* rag, const uint8_t* piece_of, bool own) {
    SindRange range_t("sind tail: SegAndMerge from the counters on, fusion, dilation, ORB mask filter");
    on_worker(p, s, worker);
    const size_t np = p->np();
    static thread_local std::vector<uint8_t> dy, lb;
    dy.resize(np); lb.resize(np);
    int r = SIND_OK;
    if (own) r = p->tails[s]->rag_half()->rag_own(&rag);      // (the slab had no room for the frame: the per-frame stage, from host planes)
    if (r == SIND_OK) r = p->tails[s]->process_end(rag, dy.data(), lb.data(), piece_of);
    if (r != SIND_OK) { sb->tail_fail.fail(s, r); return; }
    tail_finish(p, sb, o, s, t, dy, lb);
}
void tail_pieces_begin(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int g, int worker, const KmFrameResult* km, const FlowMasksReady* fm) {
    PieceBatch& pb = p->pieceb[g]; RagBatch& rb = p->ragb[g]; sind_pipe::RagRound& rr = p->ragr[g];
    int slot = -1; const int* own = nullptr; int r;
    { SindRange range_t("sind tail: flow masks, SegAndMerge up to the inputs of the piece stage");
      PhaseAOut& a = sb->a; DynaTail* tl = p->tails[s].get(); DynaTail* dh = on_worker(p, s, worker);
      const size_t np = p->np(); const int k = s * p->T + t;
      r = tl->process_begin_inputs(a.depth_h.data() + np * k, a.depth_dev.p + np * k, a.U.p + np * k, a.V.p + np * k, &a.occ[k], dh, km, fm);
      DynaTail* h = tl->rag_half();
      if (r == SIND_OK) {
          if (h->piece_batchable() && (slot = pb.take_slot()) >= 0) {
              const double tp = now_ms(); pb.pack(slot, h->piece_labels().data(), (int)h->piece_labels().size() - 1, h->piece_occ1(), h->piece_edge(), h->piece_depth_dev()); h->t_fine[10] += now_ms() - tp;
          } else {          // leaves the piece path: today's (the host function; with pieces, the per-frame RAG stage)
              slot = -1; r = h->seg_pieces_batched(nullptr, 0, nullptr, nullptr);
              if (r == SIND_OK && h->rag_pieces() > 0) { p->rag_fallback++; r = h->rag_own(&own); }
          }
      }
      if (r != SIND_OK) sb->tail_fail.fail(s, r); }
    int flush[2] = {-1, -1}, flush_n[2] = {0, 0}, nf = 0;
    { std::lock_guard<std::mutex> lk(rr.m);
      if (slot >= 0) { rr.stream_of_slot[slot] = s; const int c = pb.chunk_of(slot); if (++rr.joined[c] == pb.chunk_frames()) { flush[nf] = c; flush_n[nf++] = pb.chunk_frames(); } }
      if (++rr.arrived == rr.expected && pb.slots() > 0) {                 // the last frame of the round: the partial chunk at the end, if there is one
          const int lc = pb.chunk_of(pb.slots() - 1), n = pb.chunk_count(lc);
          if (n < pb.chunk_frames()) { flush[nf] = lc; flush_n[nf++] = n; }
      } }
    PieceChunkFrame mine; bool have_mine = false;
    for (int f = 0; f < nf; f++) {
        const double te = now_ms();
        const int first = pb.chunk_first(flush[f]), n = flush_n[f];
        std::vector<PieceChunkFrame> fr(n);
        for (int i = 0; i < n; i++) fr[i].half = p->tails[rr.stream_of_slot[first + i]]->rag_half();
        const int rc = piece_chunk_flush(pb, rb, flush[f], fr.data());
        p->tails[s]->t_fine[8] += now_ms() - te;      // (SIND_TAIL_TIMING's "rag": the flushing frame's piece and RAG launches and both waits for its whole chunk)
        const std::string e = rc == SIND_OK ? std::string() : "batched piece stage: " + std::string(sind_last_error());
        for (int i = 0; i < n; i++) {
            const int s2 = rr.stream_of_slot[first + i]; const PieceChunkFrame& q = fr[i];
            if (rc != SIND_OK) { sb->tail_fail.fail(s2, rc, e); continue; }
            if (q.fell_back) p->pieces_fallback++; else if (q.on_device) p->pieces_frames++;
            if (q.rc != SIND_OK) { sb->tail_fail.fail(s2, q.rc, q.err); continue; }
            if (q.own) p->rag_fallback++; else p->rag_frames++;
            if (s2 == s) { mine = q; have_mine = true; continue; }
            const int* res = q.rag_slot >= 0 ? rb.result(q.rag_slot) : nullptr; const uint8_t* po = q.on_device ? pb.piece_of(first + i) : nullptr; const bool ow = q.own;
            p->workers.push(sb->km_tails[g], [p, sb, o, s2, t, res, po, ow](int w) { tail_pieces_end(p, sb, o, s2, t, w, res, po, ow); });
        }
    }
    if (r != SIND_OK || !sb->tail_fail.ok(s)) return;
    if (slot < 0) { if (!own) p->rag_frames++; tail_pieces_end(p, sb, o, s, t, worker, own, nullptr, false); }
    else if (have_mine) tail_pieces_end(p, sb, o, s, t, worker, mine.rag_slot >= 0 ? rb.result(mine.rag_slot) : nullptr, mine.on_device ? pb.piece_of(slot) : nullptr, mine.own);
}
