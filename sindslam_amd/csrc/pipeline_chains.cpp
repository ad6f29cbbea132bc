// sind_pipe, phase B: the frames of a stream as chains of pool tasks (see pipeline_impl.hpp; host/pipe_schedule.hpp says when).
#include "pipeline_impl.hpp"

// One task = one frame of one stream; it queues the stream's next frame when it is done.  Frames of a stream stay in order, and the
// pool always sees up to S runnable tasks, so the workers stay busy until the end of the phase (a task per stream left the second
// "round" of 32 streams on 24 workers half empty).
// Depth half of frame k = (stream s, frame t) of a synchronous step: runs while the dense flow is on the GPU, in frame order per stream
// (the k-means warm labels are the previous frame's merged labels).  It opens the gate of the stream's next frame when it is done.
void depth_task(sind_pipe* p, StepBuf* sb, int k, int worker) {
    for (;;) {
        const int T = p->T, s = k / T, t = k % T; const size_t np = p->np();
        DynaTail* dt = depth_half(p, s); dt->stream = p->worker_streams[worker];
        const int r = dt->depth_stage(sb->a.depth_h.data() + np * k, sb->a.depth_dev.p + np * k, &sb->a.occ[k], sb->dout[k]);
        if (r != SIND_OK) sb->depth_fail.fail(k, r);
        if (!(t + 1 < T && sb->gate[k + 1].fetch_add(1) == 1)) return;
        if (p->S == 1) { k++; continue; }                    // one stream: the next frame's chain link right here (no hand-over to another worker)
        p->workers.push(sb->depth_group, [p, sb, k](int w) { depth_task(p, sb, k + 1, w); }); return;
    }
}
// Chains / FlowChains: whole tails (or flow halves behind a depth chain that ran ahead in phase A) of stream s from frame t on
void tail_task(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int worker) {
    SpinScope spin(sb->plan.inline_poll);      // one stream (whose pool workers poll anyway, pipeline_build.cpp) or a few chains on an idle host
    for (;;) {
        if (!tail_one(p, sb, o, s, t, worker, nullptr) || t + 1 >= sb->range(s, p->T).t1) return;
        if (sb->plan.inline_poll) { t++; continue; }       // the next frame's chain link right here (no hand-over to another worker)
        p->workers.push(sb->tail_group, [p, sb, o, s, t](int w) { tail_task(p, sb, o, s, t + 1, w); }); return;
    }
}
// Two chains per stream for a handful of live streams (the slow runners of a repair): the depth chain -- k-means from the previous frame's merged labels, SegAndMerge; it
// needs nothing from the flow half -- runs ahead on the stream's depth-half object, the flow chain (flow masks, fusion, dilation, keypoint filter) follows frame by frame
// as soon as its frame's depth stage and the previous frame's flow stage are done.  A frame then costs max(depth, flow) instead of their sum (the in-order mode's schedule).
// Split rounds end in the same flow chains: there a round's task runs the frame's depth stage.
void flow_chain(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t, int t1, int worker) {
    SpinScope spin(sb->plan.inline_poll);      // (a few chains on an idle host poll before they sleep; the rounds of a full pipeline do not)
    for (;;) {
        if (!tail_one(p, sb, o, s, t, worker, nullptr) || t + 1 >= t1) return;
        if (sb->fgate[s * p->T + t + 1].fetch_add(1) != 1) return;          // the next frame's depth stage is still out: its completion starts the flow stage
        t++;
    }
}
void depth_chain(sind_pipe* p, StepBuf* sb, PipeOut o, int s, int t0, int t1, int worker) {
    SpinScope spin(true);
    const size_t np = p->np();
    DynaTail* dt = p->dtails[s].get(); dt->stream = p->worker_streams[worker];
    for (int t = t0; t < t1; t++) {
        const int k = s * p->T + t;
        const int r = dt->depth_stage(sb->a.depth_h.data() + np * k, sb->a.depth_dev.p + np * k, &sb->a.occ[k], sb->dout[k], nullptr);
        if (r != SIND_OK) { sb->dchain_fail.fail(s, r); return; }      // the flow chain of this stream stops at the frame before
        if (sb->fgate[k].fetch_add(1) == 1) p->workers.push(sb->tail_group, [p, sb, o, s, t, t1](int w) { flow_chain(p, sb, o, s, t, t1, w); });
    }
}
// Gates of a step's flow chains: a frame's flow stage starts when its depth stage and the stream's previous flow stage are both done (a stream's first frame waits
// for its depth stage only).  Gates outside a stream's frame range are set too and never read.
void arm_flow_gates(sind_pipe* p, StepBuf& sb) {
    const int B = p->S * p->T;
    if (sb.fgate_n < B) { sb.fgate.reset(new std::atomic<int>[B]); sb.fgate_n = B; }
    sb.dout.assign(B, DepthStageOut());
    for (int s = 0; s < p->S; s++) { const int t0 = sb.range(s, p->T).t0; for (int t = 0; t < p->T; t++) sb.fgate[s * p->T + t].store(t == t0 ? 1 : 0); }
}
