// sind_pipe: phase A of a step -- the state-free batch over S x T frames (see pipeline_impl.hpp).
#include "pipeline_impl.hpp"

// ---- CalOccluded of every frame (state free: depth only) on the pool, concurrent with the dense flow (the host cores would otherwise idle while the GPU runs the flow solver)
// frame k has its CalOccluded result (or its error): open the depth chain's gate
static void occ_done(sind_pipe* p, StepBuf* sb, int k, int rc) {
    if (rc != SIND_OK) sb->occ_fail.fail(k, rc);
    if (sb->depth_ahead && sb->gate[k].fetch_add(1) == 1) p->workers.push(sb->depth_group, [p, sb, k](int w) { depth_task(p, sb, k, w); });
}
static OccGpuOut occ_pre(sind_pipe* p, StepBuf* sb, int k) {
    const size_t np = p->np(), nblk = (size_t)(p->c.width / 16) * (p->c.height / 16);
    return OccGpuOut{sb->occ_edge_h.data() + np * k, sb->occ_total_h.data() + np * k, sb->occ_blocks_h.data() + nblk * k, sb->occ_edge_h.data() + np * k /* the edge image has been packed by then */, sb->occ2_ev[k]};
}
static void grow_skip(StepBuf* sb, int k) { const PeacGrowHdr skip{0, 0, 1, k}; std::memcpy(sb->grow_in_h.p + (size_t)k * PG_IN_STRIDE, &skip, sizeof(skip)); }      // the grow kernel passes frame k over
// first halves: GPU stencil results of the frame's chunk -> end points, PEAC graph clustering, the grow's input block; the runner that completes a chunk
// enqueues its region grow (one launch for the chunk's frames; the launches share one device workspace, hence the lock around the enqueue)
static void occ_first_halves(sind_pipe* p, StepBuf* sb, int B, int w) {
    PhaseAOut& a = sb->a; const size_t np = p->np(), PP = (size_t)PEAC_GROW_MAX_PLANES * PEAC_GROW_MAX_PLANES;
    for (int k; (k = sb->occ_next.fetch_add(1)) < B;) {
        SindRange r("sind CalOccluded, first half: end points, PEAC graph");
        const int ch = k / p->occ_chunk; int rc = SIND_OK;
        if (sind_event_wait(sb->occ_ev[ch]) != hipSuccess) { (void)hipGetLastError(); sind_set_error("batched CalOccluded stage failed"); rc = SIND_E_HIP; }
        else {
            const OccGpuOut pre = occ_pre(p, sb, k);
            const bool on_gpu = ((k + 1) * sb->grow_q) / 4 > (k * sb->grow_q) / 4;          // grow_q of every four frames
            rc = p->occ_tails[w]->compute_occluded_p1(a.depth_h.data() + np * k, a.depth_dev.p + np * k, sb->occ_ctx[k], &pre, on_gpu ? sb->grow_in_h.p + (size_t)k * PG_IN_STRIDE : nullptr, k);
            if (!on_gpu) grow_skip(sb, k);      // grown on the host in the first half
        }
        if (rc != SIND_OK) { sb->occ_fail.fail(k, rc); grow_skip(sb, k); }
        if (sb->grow_left[ch].fetch_sub(1) != 1) continue;
        const int c0 = ch * p->occ_chunk, nb = std::min(p->occ_chunk, B - c0); int lrc = SIND_OK;
        if (sb->grow_q == 0) { sb->grow_state[ch].store(2); continue; }         // every frame of the chunk grew on the host: nothing to launch (state 2)
        { std::lock_guard<std::mutex> lk(p->grow_mu);
          lrc = p->grow.run(p->grow_stream, sb->grow_in_h.p + (size_t)c0 * PG_IN_STRIDE, a.depth_dev.p, nb, sb->grow_member_h.p + np * c0, sb->grow_pair_h.p + PP * c0, sb->grow_status_h.p + 4 * c0);
          if (lrc == SIND_OK && hipEventRecord(sb->grow_ev[ch], p->grow_stream) != hipSuccess) lrc = SIND_E_HIP; }
        sb->grow_state[ch].store(lrc == SIND_OK ? 1 : -1);
    }
}
// second halves, in frame order: wait for the chunk's grow, then PEAC's last merge, plane contours, contour filter, closing
static void occ_second_halves(sind_pipe* p, StepBuf* sb, int B, int w) {
    const size_t np = p->np(), PP = (size_t)PEAC_GROW_MAX_PLANES * PEAC_GROW_MAX_PLANES;
    for (int k; (k = sb->occ_next2.fetch_add(1)) < B;) {
        SindRange r("sind CalOccluded, second half: plane contours, contour filter");
        const int ch = k / p->occ_chunk;
        // grow_state[ch] is set behind EVERY first half of the chunk (grow_left): only after this wait is frame k's failure slot final
        if (sb->grow_state[ch].load() == 0) { SindTokenPause pause; while (sb->grow_state[ch].load() == 0) std::this_thread::sleep_for(std::chrono::microseconds(50)); }
        if (sb->occ_fail.ok(k)) {
            const int gs = sb->grow_state[ch].load(); int rc;
            if (gs < 0 || (gs == 1 && sind_event_wait(sb->grow_ev[ch]) != hipSuccess)) { (void)hipGetLastError(); sind_set_error("PEAC region grow (chunk %d) failed", ch); rc = SIND_E_HIP; }
            else { const OccGpuOut pre = occ_pre(p, sb, k); rc = p->occ_tails[w]->compute_occluded_p2(sb->occ_ctx[k], sb->grow_member_h.p + np * k, sb->grow_pair_h.p + PP * k, sb->grow_status_h.p + 4 * k, sb->a.occ[k], &pre); }
            if (rc != SIND_OK) sb->occ_fail.fail(k, rc);
        }
        sb->occ_ctx[k] = OccCtx();
        occ_done(p, sb, k, SIND_OK);              // (an error of this frame has been recorded above)
    }
}
// `occ_workers` runner tasks share the frames through a counter: CalOccluded is host-heavy (PEAC region grow), and more runnable
// threads than the CPU quota of the box (cgroup cpu.max, 16 cores per GPU) only burn the quota early in a period and stall EVERY
// thread of the process, the flow's launch threads included, until the period ends
static void push_occ_runners(sind_pipe* p, StepBuf* sb, int B) {
    for (int r = 0; r < std::min(p->occ_workers, B); r++) p->workers.push(sb->occ_group, [p, sb, B](int w) {
        if (p->batch_occ) { occ_first_halves(p, sb, B, w); occ_second_halves(p, sb, B, w); return; }
        const size_t np = p->np();       // per-frame path: GPU and host half of a frame in one call
        for (int k; (k = sb->occ_next.fetch_add(1)) < B;) occ_done(p, sb, k, p->occ_tails[w]->compute_occluded(sb->a.depth_h.data() + np * k, sb->a.depth_dev.p + np * k, sb->a.occ[k]));
    });
}
// GPU half of CalOccluded, chunk by chunk, behind the depth copies; the counters of the runners
static int occ_begin(sind_pipe* p, StepBuf& sb, int B) {
    const int W = p->c.width, H = p->c.height; const size_t np = p->np(), nblk = (size_t)(W / 16) * (H / 16); PhaseAOut& a = sb.a;
    a.occ.assign(B, OccResult());
    for (int k = 0; k < B; k++) { a.occ[k].occ2_dev = a.occ2_dev.p + np * k; a.occ[k].depthN_dev = a.depthN_dev.p + np * k; }
    sb.occ_fail.reset(B);
    sb.occ_next.store(0); sb.occ_next2.store(0); sb.grow_q = p->grow_ok ? p->grow_q : 0;
    if (!p->batch_occ) return SIND_OK;
    HIP_TRY(hipStreamWaitEvent(p->occ_stream, p->ev_depth, 0));
    for (int c0 = 0, c = 0; c0 < B; c0 += p->occ_chunk, c++) {
        const int nb = std::min(p->occ_chunk, B - c0);
        SIND_TRY(p->occb.run(p->occ_stream, a.depth_dev.p + np * c0, nb, a.depthN_dev.p + np * c0, sb.occ_edge_h.data() + np * c0, sb.occ_total_h.data() + np * c0, sb.occ_blocks_h.data() + nblk * c0));
        HIP_TRY(hipEventRecord(sb.occ_ev[c], p->occ_stream));
        sb.grow_left[c].store(nb); sb.grow_state[c].store(0);
    }
    sb.occ_ctx.clear(); sb.occ_ctx.resize(B);
    return SIND_OK;
}

// ---- dense flow for every (n, n-2) pair, second pass for large-motion pairs, refinement, up-scale.  The batch may be cut into slices that run the whole flow pyramid
// concurrently on their own streams (SIND_FLOW_SPLIT): launches of different slices overlap on the GPU, so one slice's load phase can hide under another slice's iterations
struct FlowSlices {
    int nsl, Bs; size_t gsz; std::vector<DynaFront*> fr; std::vector<int> cur, p1, p2; Failures fail;
    std::vector<double> ms, other_ms; std::vector<std::vector<std::pair<double, double>>> iv;
};
static void run_flow_slice(sind_pipe* p, StepBuf& sb, FlowSlices& fs, int B, int i) {
    const int W = p->c.width, H = p->c.height, b0 = i * fs.Bs, nb = std::min(fs.Bs, B - b0); if (nb <= 0) return;
    const size_t np = p->np(), gsz = fs.gsz; PhaseAOut& a = sb.a;
    SindRange r("sind dense flow slice: DeepFlow, large-motion pass, refinement, up-scale");
    DynaFront& f = *fs.fr[i]; f.flow.sor_timer.enabled = true; f.flow.sor_timer.reset();
    if (i > 0 && hipStreamWaitEvent(f.stream, p->ev_pool, 0) != hipSuccess) { fs.fail.fail(i, SIND_E_HIP, "hipStreamWaitEvent failed"); return; }
    int rc = f.dense_flow(p->pool.p, fs.cur.data() + b0, fs.p1.data() + b0, fs.p2.data() + b0, nb, a.U.p + np * b0, a.V.p + np * b0, a.large_motion.data() + b0);      // the slices' flag ranges are disjoint: no lock
    if (rc == SIND_OK) {       // sample grid of the slice's frames for the tails' PROSAC pairs: one launch + one copy instead of one each per frame
        rc = launch_gather_grid(f.stream, a.U.p + np * b0, a.V.p + np * b0, a.grid_dev.p + gsz * b0, W, H, 10, nb);
        if (rc == SIND_OK && hipMemcpyAsync(a.grid_h.p + gsz * b0, a.grid_dev.p + gsz * b0, gsz * nb * sizeof(float), hipMemcpyDeviceToHost, f.stream) != hipSuccess) rc = SIND_E_HIP;
    }
    if (rc == SIND_OK && sind_stream_wait(f.stream) != hipSuccess) rc = SIND_E_HIP;
    if (rc != SIND_OK) { fs.fail.fail(i, rc); return; }
    // the slice reads its own event brackets (three hipEventElapsedTime per bracket, ~150 brackets) while the other slices still run
    fs.ms[i] = f.flow.sor_timer.collect_ms(0); fs.other_ms[i] = f.flow.sor_timer.collect_ms(1); f.flow.sor_timer.intervals(p->ev_pool, fs.iv[i], 0);
}
// length of the union of intervals: the time during which at least one slice had solver launches in flight
static double union_length(std::vector<std::pair<double, double>>& iv) {
    std::sort(iv.begin(), iv.end()); double un = 0, cs = 0, ce = -1;
    for (const auto& q : iv) { if (q.first > ce) { if (ce > cs) un += ce - cs; cs = q.first; ce = q.second; } else ce = std::max(ce, q.second); }
    return ce > cs ? un + ce - cs : un;
}
static void collect_solver_stats(sind_pipe* p, FlowSlices& fs) {
    p->sor_ms = 0; p->sor_bytes = 0; p->sor_launches = 0; p->sor_slices = fs.nsl; p->sor_other_ms = 0; p->sor_other_bytes = 0; p->sor_other_launches = 0;
    std::vector<std::pair<double, double>> iv;
    for (int i = 0; i < fs.nsl; i++) { const auto& tm = fs.fr[i]->flow.sor_timer; p->sor_ms += fs.ms[i]; p->sor_bytes += tm.alg_bytes; p->sor_launches += tm.launches;
        p->sor_other_ms += fs.other_ms[i]; p->sor_other_bytes += tm.alg_bytes_other; p->sor_other_launches += tm.launches_other; iv.insert(iv.end(), fs.iv[i].begin(), fs.iv[i].end()); }
    p->sor_union_ms = union_length(iv);
}
// one host thread per slice; once the slices are on their way, waits for the depth copies and starts the CalOccluded runners from here
static int dense_flow_slices(sind_pipe* p, StepBuf& sb, int B) {
    const int S = p->S, T = p->T, nsl = 1 + (int)p->extra_fronts.size();
    FlowSlices fs{nsl, (B + nsl - 1) / nsl, p->gsz()};
    fs.cur.resize(B); fs.p1.resize(B); fs.p2.resize(B); fs.fail.reset(nsl); fs.ms.assign(nsl, 0.0); fs.other_ms.assign(nsl, 0.0); fs.iv.resize(nsl);
    for (int s = 0; s < S; s++) for (int tt = 0; tt < T; tt++) { const int k = s * T + tt, base = s * (T + 2) + tt; fs.cur[k] = base + 2; fs.p1[k] = base + 1; fs.p2[k] = base; }
    sb.a.large_motion.assign(B, 0);
    fs.fr.assign(1, &p->front); for (auto& f : p->extra_fronts) fs.fr.push_back(f.get());
    HIP_TRY(hipEventRecord(p->ev_pool, p->stream));
    std::vector<std::thread> th;
    for (int i = 0; i < nsl; i++) th.emplace_back([&, i] { (void)pthread_setname_np(pthread_self(), "sind-flow"); (void)hipSetDevice(p->c.device); run_flow_slice(p, sb, fs, B, i); g_cpu_us_flow += (long long)(thread_cpu_ms() * 1e3); });
    g_cpu_steps++;
    const hipError_t depth_ok = sind_event_wait(p->ev_depth);
    if (depth_ok == hipSuccess) push_occ_runners(p, &sb, B);
    for (auto& slice_thread : th) slice_thread.join();
    if (depth_ok != hipSuccess) { (void)hipGetLastError(); sind_set_error("copy of the depth frames failed"); return SIND_E_HIP; }
    SIND_TRY(fs.fail.first_error("dense flow slice %d: %s"));
    for (int k = 0; k < B; k++) sb.a.occ[k].gridFlow = sb.a.grid_h.p + fs.gsz * k;
    collect_solver_stats(p, fs);
    return SIND_OK;
}

// gray for all frames, 0.6-scaled gray into the per-stream pools behind the two history slots; *gray_for_orb: the image the ORB front reads
static int gray_and_resize(sind_pipe* p, const uint8_t* bgr_dev, int B, const uint8_t** gray_for_orb) {
    SindRange range_front("sind front: gray + 0.6 resize");
    const int W = p->c.width, H = p->c.height; const size_t np = p->np(), fb = (size_t)p->fw * p->fh;
    *gray_for_orb = p->gray.p;
    SIND_TRY(launch_bgr2gray(p->stream, bgr_dev, p->gray.p, np * B, false));
    // frame t of stream s goes to pool slot s * (T + 2) + 2 + t: one launch, T frames per group, two history slots skipped between the groups
    SIND_TRY(launch_resize_u8(p->stream, p->gray.p, p->pool.p + fb * 2, W, H, p->fw, p->fh, B, W, p->fw, np, fb, p->T, 2));
    if (p->c.orb_gray_rgb_order) { SIND_TRY(launch_bgr2gray(p->stream, bgr_dev, p->gray_orb.p, np * B, true)); *gray_for_orb = p->gray_orb.p; }
    HIP_TRY(hipEventRecord(p->ev_gray, p->stream));
    return SIND_OK;
}
// roll the gray history: the last two frames of every stream become slots 0, 1 (one launch; the flow grid is a multiple of 16 bytes for every
// supported size -- width % 64 == 0 -- and the copy-per-stream path stays for anything else)
static int roll_gray_history(sind_pipe* p) {
    const int S = p->S, T = p->T; const size_t fb = (size_t)p->fw * p->fh;
    if (fb % 16 == 0) return launch_roll_history(p->stream, p->pool.p, S, T, fb);
    for (int s = 0; s < S; s++) {
        uint8_t* base = p->pool.p + fb * (size_t)s * (T + 2);
        if (T >= 2) { HIP_TRY(hipMemcpyAsync(base, base + fb * T, fb * 2, hipMemcpyDeviceToDevice, p->stream)); }
        else { HIP_TRY(hipMemcpyAsync(base, base + fb, fb, hipMemcpyDeviceToDevice, p->stream)); HIP_TRY(hipMemcpyAsync(base + fb, base + fb * 2, fb, hipMemcpyDeviceToDevice, p->stream)); }
    }
    return SIND_OK;
}

// ---- phase A of one step (state free, batched over S*T frames, shared HIP stream): fills a StepBuf
int phase_a(sind_pipe* p, StepBuf& sb, const uint8_t* bgr_dev, const uint16_t* depth_dev, double t[4], bool depth_ahead) {
    const int T = p->T, B = p->S * T; const size_t np = p->np(); PhaseAOut& a = sb.a;
    t[0] = now_ms();
    SindRange range_a("sind phase A (state-free: gray, dense flow, ORB front, CalOccluded)");
    const uint8_t* gray_for_orb = nullptr;
    SIND_TRY(gray_and_resize(p, bgr_dev, B, &gray_for_orb));
    // private copies of the depth frames: device (tail kernels of this step run while the caller may reuse its buffer) and host.  They go
    // ahead of the ORB front on its stream (157 MB to the host, ~3 ms): the flow slices need not wait for them, only the CalOccluded tasks do
    HIP_TRY(hipMemcpyAsync(a.depth_dev.p, depth_dev, np * B * sizeof(uint16_t), hipMemcpyDeviceToDevice, p->orb_stream));
    HIP_TRY(hipMemcpyAsync(a.depth_h.data(), a.depth_dev.p, np * B * sizeof(uint16_t), hipMemcpyDeviceToHost, p->orb_stream));
    HIP_TRY(hipEventRecord(p->ev_depth, p->orb_stream));
    // ORB front (pyramid, FAST, octree, orientation, blur, BRIEF) of all frames: independent of the flow, so it runs on its own HIP
    // stream and host thread underneath the dense flow instead of after it
    int orb_rc = SIND_OK; std::string orb_err;
    std::thread orb_thread([&] {
        (void)pthread_setname_np(pthread_self(), "sind-orb");
        (void)hipSetDevice(p->c.device);
        if (hipStreamWaitEvent(p->orb_stream, p->ev_gray, 0) != hipSuccess) { orb_rc = SIND_E_HIP; orb_err = "hipStreamWaitEvent failed"; return; }
        { SindRange r("sind ORB front: pyramid, FAST, octree, orientation, BRIEF"); orb_rc = p->orb.extract_all(gray_for_orb, B, a.orb); }
        if (orb_rc != SIND_OK) orb_err = sind_last_error();
        g_cpu_us_orb += (long long)(thread_cpu_ms() * 1e3); });
    struct OrbJoin { std::thread& t; ~OrbJoin() { if (t.joinable()) t.join(); } } orb_join{orb_thread};
    SIND_TRY(a.alloc(np, B, p->gsz()));      // the first step of this set: what construction left out
    SIND_TRY(occ_begin(p, sb, B));
    struct Waiter { TaskGroup& g; ~Waiter() { WorkerPool::wait(g); } };       // no task may outlive this call's buffers on an error return
    Waiter depth_waiter{sb.depth_group}, waiter{sb.occ_group};                // destroyed in reverse order: CalOccluded runners first (they open the last gates), then the depth chains
    sb.depth_ahead = depth_ahead;
    if (depth_ahead) {
        sb.dout.assign(B, DepthStageOut()); sb.depth_fail.reset(B);
        if (!sb.gate) sb.gate.reset(new std::atomic<int>[B]);
        for (int k = 0; k < B; k++) sb.gate[k].store(k % T == 0 ? 1 : 0);       // the first frame of a stream only waits for its CalOccluded
    }
    t[1] = now_ms();
    SIND_TRY(dense_flow_slices(p, sb, B));
    t[2] = now_ms();
    orb_thread.join();
    if (orb_rc != SIND_OK) { sind_set_error("ORB front: %s", orb_err.c_str()); return orb_rc; }
    SIND_TRY(roll_gray_history(p));
    HIP_TRY(sind_stream_wait(p->stream));
    WorkerPool::wait(sb.occ_group);
    WorkerPool::wait(sb.depth_group);           // every chain has been started by now (a gate is opened from inside a running task of either group)
    SIND_TRY(sb.occ_fail.first_error("stream %d (CalOccluded): %s", T));
    if (depth_ahead) SIND_TRY(sb.depth_fail.first_error("stream %d (depth stage): %s", T));
    t[3] = now_ms();
    sb.active.swap(p->active_next); p->active_next.clear(); sb.first.clear();           // applies to this step only
    sb.retain_tag = p->retain_tag_next; p->retain_tag_next = -1;
    sb.state_hash.assign((size_t)2 * B, 0);
    sb.pending = true;
    return SIND_OK;
}
