"""GPU: every schedule of the batched pipeline's phase B (sindslam_amd/csrc/host/pipe_schedule.hpp), reached on purpose and asserted through Pipeline.last_schedule():
the two steps of motion_scene.py's small configurations equal the oracle frame for frame whichever schedule ran them; a ragged step gives the same outputs, state
fingerprints and state blobs as two chains and as rounds; a retained step replayed over per-stream frame ranges runs as two chains and repeats the synchronous results."""
import numpy as np
import pytest

import motion_scene as M
from test_pipeline_motion_gpu import _check_flags, _check_frame, _pipeline, _step

pytestmark = pytest.mark.gpu

ROWS = [  # configuration, constructor arguments, depth-ahead, the schedule both steps must report
    ("one_slice", {}, False, "split_rounds"),                          # default pool: no more streams than workers
    ("one_slice", dict(host_threads=2), False, "rounds"),              # more streams than workers
    ("one_slice", dict(flow_opts_off=16), False, "rounds"),            # split switched off
    ("one_slice", {}, True, "flow_chains"),                            # synchronous steps with the depth chain run ahead in phase A
    ("one_one", {}, False, "chains"),                                  # one stream
]


def _frame(pipe, s, t):
    k, d = pipe.keypoints(s, t)
    return pipe.dyna[s, t].copy(), pipe.label[s, t].copy(), pipe.mask[s, t].copy(), k.tobytes(), d.copy()


def _same(a, b, what):
    for i in (0, 1, 2, 4):
        assert np.array_equal(a[i], b[i]), (what, i)
    assert a[3] == b[3], (what, "keypoints")


@pytest.mark.parametrize("name,kw,ahead,want", ROWS, ids=["default", "two_workers", "split_off", "depth_ahead", "one_stream"])
def test_two_steps_equal_the_oracle_on_the_schedule_they_report(name, kw, ahead, want):
    from sindslam_amd._lib import SindError
    pipe, data = _pipeline(name, **kw)
    try:
        if not kw:
            assert pipe.host_info()["workers"] >= pipe.S           # the default pool of any supported host holds these few streams
        with pytest.raises(SindError, match="no step has finished"):
            pipe.last_schedule()
        if ahead:
            pipe.set_depth_ahead(True)
        for step in range(M.STEPS):
            lo = _step(pipe, data, step)
            assert pipe.last_schedule() == want, step
            _check_flags(pipe, name, lo, (want, step))
            for s in range(pipe.S):
                for t in range(pipe.T):
                    _check_frame(pipe, name, s, t, lo + t, (want, step))
    finally:
        pipe.close()


def test_ragged_step_as_two_chains_and_as_rounds():
    """a full step, then set_active_frames([2, 1, 0, 2]): two chains with the default chain_max_streams, rounds with 0 (split with the default pool, non-split with
    two workers); the frames that ran equal the oracle, and outputs, state fingerprints and state blobs are the same on all three"""
    name = M.RAGGED; act = [2, 1, 0, 2]; got = {}
    for want, cmax, kw in (("two_chains", None, {}), ("split_rounds", 0, {}), ("rounds", 0, dict(host_threads=2))):
        pipe, data = _pipeline(name, **kw)
        try:
            pipe.set_state_hashing(True)
            if cmax is not None:
                pipe.set_chain_max_streams(cmax)
            _step(pipe, data, 0)
            assert pipe.last_schedule() == ("rounds" if kw else "split_rounds")
            pipe.set_active_frames(np.array(act, np.int32))
            lo = _step(pipe, data, 1)
            assert pipe.last_schedule() == want
            frames = {}
            for s in range(pipe.S):
                for t in range(act[s]):
                    _check_frame(pipe, name, s, t, lo + t, (want, "ragged")); frames[s, t] = _frame(pipe, s, t)
            got[want] = (frames, pipe.state_hashes(), [pipe.get_state(s) for s in range(pipe.S)])
        finally:
            pipe.close()
    ref = got["two_chains"]
    assert all(ref[1][s, t].any() == (t < act[s]) for s in range(4) for t in range(2))          # a fingerprint for exactly the frames that ran
    for want in ("split_rounds", "rounds"):
        frames, hashes, blobs = got[want]
        for key in ref[0]:
            _same(ref[0][key], frames[key], (want, key))
        assert np.array_equal(ref[1], hashes), want
        for s in range(4):
            assert np.array_equal(ref[2][s], blobs[s]), (want, "state of stream", s)


def test_replay_of_a_retained_step_runs_as_two_chains():
    """the first step kept, then its tails again from restored states: all streams up to frame 1, then stream s over [first[s], last[s]) -- two chains both times, and
    every frame that ran repeats the synchronous step's outputs and fingerprints"""
    name = "one_slice"; pipe, data = _pipeline(name); S, T = pipe.S, pipe.T
    try:
        pipe.set_state_hashing(True); pipe.reserve_retained(1)
        start = [pipe.get_state(s) for s in range(S)]
        pipe.retain_next(7)
        lo = _step(pipe, data, 0)
        assert pipe.last_schedule() == "split_rounds"
        sync = {(s, t): _frame(pipe, s, t) for s in range(S) for t in range(T)}; sync_hash = pipe.state_hashes()
        for s in range(S):
            _check_frame(pipe, name, s, 0, lo, "synchronous")

        def replay(first, last, states):
            for s in range(S):
                pipe.set_state(s, states[s])
            pipe.replay(7, first, last)
            assert pipe.last_schedule() == "two_chains", (first, last)
            h = pipe.state_hashes()
            for s in range(S):
                for t in range(T):
                    if first[s] <= t < last[s]:
                        _same(sync[s, t], _frame(pipe, s, t), ("replay", first, last, s, t)); assert np.array_equal(h[s, t], sync_hash[s, t]), (s, t)
                    else:
                        assert not h[s, t].any(), (s, t)

        replay([0] * S, [1] * S, start)
        after0 = [pipe.get_state(s) for s in range(S)]
        first, last = [0, 1, 2, 0], [2, 2, 2, 1]
        replay(first, last, [after0[s] if first[s] == 1 else start[s] for s in range(S)])
    finally:
        pipe.close()
