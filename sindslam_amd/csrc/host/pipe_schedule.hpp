#pragma once
// Which schedule the stateful tails of a sind_pipe step take: phase_b_start asks once per step and keeps the answer in the step buffer.
// Nothing from HIP: libsind_host.so exports it (sindh_pipe_schedule), tests/test_pipe_schedule_cpu.py holds the table.
namespace sind {

enum class TailSchedule : int {
    Chains = 0,        // one chain per stream over whole tails
    FlowChains = 1,    // ... over flow halves: the depth chain ran ahead in phase A (depth-ahead)
    TwoChains = 2,     // few live streams: per stream a depth chain ahead of a flow chain
    Rounds = 3,        // frame t of every stream: batched k-means, flow masks, RAG; then the tails on the pool
    SplitRounds = 4    // rounds that wait for the depth halves only; flow halves as chains, k-means the one batched stage
};
struct TailPlan { TailSchedule kind; bool inline_poll; };      // inline_poll: chains run the stream's next frame in the same task and poll the GPU before they sleep

// ragged: per-stream frame ranges (set_active_frames, replay); nact: streams whose range is not empty.  Few live streams run as chains with their own k-means
// launches: a round costs ~60 dependent launches per frame whatever the batch, and its barrier waits for the slowest tail.  Split rounds only while there are
// no more streams than pool workers (with more, other streams' tails fill the pool during a round anyway).
inline TailPlan tail_schedule(int S, int workers, bool batch_km, bool depth_ahead, bool split_rounds, int chain_max_streams, bool ragged, int nact) {
    const bool few = ragged && nact <= chain_max_streams, inline_poll = S == 1 || few;
    if (few && S > 1 && !depth_ahead) return {TailSchedule::TwoChains, inline_poll};
    if (batch_km && !depth_ahead && !few) return {split_rounds && S <= workers ? TailSchedule::SplitRounds : TailSchedule::Rounds, inline_poll};
    return {depth_ahead ? TailSchedule::FlowChains : TailSchedule::Chains, inline_poll};
}
// what a step falls back to when the depth-half objects it needs cannot be created
inline TailSchedule without_depth_halves(TailSchedule k) { return k == TailSchedule::TwoChains ? TailSchedule::Chains : k == TailSchedule::SplitRounds ? TailSchedule::Rounds : k; }
// the tails of this schedule find their frame's depth stage done and run the flow stage only
inline bool runs_flow_halves(TailSchedule k) { return k == TailSchedule::FlowChains || k == TailSchedule::TwoChains || k == TailSchedule::SplitRounds; }

}  // namespace sind
