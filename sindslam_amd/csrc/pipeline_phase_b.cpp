// sind_pipe: phase B of a step -- which schedule its stateful tails take (host/pipe_schedule.hpp), their start and their end (see pipeline_impl.hpp).
#include "pipeline_impl.hpp"

// Chains / FlowChains: one chain per stream that has frames in this step
static void start_chains(sind_pipe* p, StepBuf* sb, const PipeOut& o) {
    for (int s = 0; s < p->S; s++) {
        const StepBuf::Frames f = sb->range(s, p->T);
        if (f.t0 < f.t1) p->workers.push(sb->tail_group, [p, sb, o, s, f](int w) { tail_task(p, sb, o, s, f.t0, w); });
    }
}
// TwoChains: per stream a depth chain; it starts the stream's flow chain behind its first frame (pipeline_chains.cpp)
static void start_two_chains(sind_pipe* p, StepBuf* sb, const PipeOut& o) {
    arm_flow_gates(p, *sb);
    for (int s = 0; s < p->S; s++) {
        const StepBuf::Frames f = sb->range(s, p->T);
        if (f.t0 < f.t1) p->workers.push(sb->tail_group, [p, sb, o, s, f](int w) { depth_chain(p, sb, o, s, f.t0, f.t1, w); });
    }
}
void phase_b_start(sind_pipe* p, StepBuf& sb, const PipeOut& o) {
    const int S = p->S;
    sb.tail_fail.reset(S); sb.dchain_fail.reset(S);
    int nact = 0; for (int s = 0; s < S; s++) { const StepBuf::Frames f = sb.range(s, p->T); nact += f.t0 < f.t1; }
    sb.plan = tail_schedule(S, (int)p->worker_streams.size(), p->batch_km, sb.depth_ahead, p->split_rounds, p->chain_max_streams, sb.ragged(), nact);
    if (sb.plan.kind != without_depth_halves(sb.plan.kind) && ensure_dtails(p) != SIND_OK) sb.plan.kind = without_depth_halves(sb.plan.kind);
    switch (sb.plan.kind) {
        case TailSchedule::Chains: case TailSchedule::FlowChains: start_chains(p, &sb, o); break;
        case TailSchedule::TwoChains: start_two_chains(p, &sb, o); break;
        case TailSchedule::SplitRounds: arm_flow_gates(p, sb);      // fall through
        case TailSchedule::Rounds: start_rounds(p, &sb, o); break;
    }
}
int phase_b_finish(sind_pipe* p, StepBuf& sb) {
    for (std::thread& t : p->round_threads) if (t.joinable()) t.join();
    p->round_threads.clear();
    for (TaskGroup& g : sb.km_tails) WorkerPool::wait(g);      // (first: with split rounds a depth half queues its frame's flow half into tail_group when it is done)
    WorkerPool::wait(sb.tail_group);
    sb.pending = false;
    p->last_hash = sb.state_hash; p->last_large_motion = sb.a.large_motion; p->last_schedule = (int)sb.plan.kind;
    if (sb.retain_tag >= 0) {                       // keep this step's phase-A outputs: they change places with a reserve set of the same sizes
        if (p->spare.empty()) { sind_set_error("sind_pipe: no reserve left to retain step %d (sind_pipe_reserve_retained)", sb.retain_tag); sb.retain_tag = -1; return SIND_E_STATE; }
        std::unique_ptr<sind_pipe::Retained> r = std::move(p->spare.back()); p->spare.pop_back();
        sb.a.swap(r->a); r->tag = sb.retain_tag; sb.retain_tag = -1;
        for (OccResult& o : r->a.occ) o.occ2_event = nullptr;            // the uploads behind these events are long done; the events belong to the step buffer and are recorded again
        p->kept.push_back(std::move(r));
    }
    const int rc = sb.tail_fail.first_error("stream %d: %s");
    return rc != SIND_OK ? rc : sb.dchain_fail.first_error("stream %d (depth chain): %s");
}
int phase_b(sind_pipe* p, StepBuf& sb, const PipeOut& o) { phase_b_start(p, sb, o); return phase_b_finish(p, sb); }
