"""GPU: the batched pipeline with SegAndMerge's piece extraction batched per round on the GPU (set_pieces_batch), against the oracle and against the same run with
the switch off: Pipeline(4, 2) at 192 x 144 on four depth kinds, in the non-split `rounds` schedule, with chunks of 3 + 1 and with the default chunk.  pieces_batch()
must report every frame cut by the batched stage and none fallen back: an equal result through a silent fallback would prove nothing.  Where the round does not run
-- the batched RAG stage off, a replayed step that takes chains -- the switch changes nothing and its counters stay 0.  A ragged step completes its partial chunk."""
import numpy as np
import pytest

import depth_ref as R
import depth_scene as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

W, H = 192, 144
ORB = (1000, 1.2, 8, 15, 5)
CASE = {}


def case():
    """frames, the four depth kinds, intrinsics and the oracle's stages: computed once, never changed"""
    if not CASE:
        bgr, plain, K = S.stream_case(W, H, "plain")
        depths = [plain, S.stream_case(W, H, "steps")[1], S.stream_case(W, H, "speckle")[1], S.stream_case(W, H, "lowrange")[1]]
        CASE.update(bgr=bgr, depths=depths, K=K, refs=[R.oracle_stages(bgr, d, K) for d in depths])
    return CASE["bgr"], CASE["depths"], CASE["K"], CASE["refs"]


def make_pipe(on, chunk=None, rag_batch=True):
    from sindslam_amd.pipeline import Pipeline
    bgr, depths, K, _ = case()
    # four streams are fewer than the pool has workers, where a step would take split rounds: bit 4 of flow_opts_off (an A/B switch, same results) makes them whole
    # rounds, the schedule of a step with more streams than workers and the only one the batched piece stage is part of
    pipe = Pipeline(4, 2, W, H, *K, *ORB, orb_gray_rgb_order=1, flow_opts_off=16)
    pipe.set_chain_max_streams(0); pipe.set_rag_batch(rag_batch)
    if chunk is not None:
        pipe.set_rag_batch_chunk(chunk)
    assert pipe.pieces_batch() == (False, 0, 0)
    pipe.set_pieces_batch(on)
    for s in range(4):
        pipe.prime(s, bgr[1], bgr[0])
    return pipe


def step(pipe):
    bgr, depths, _, _ = case()
    pipe.process(np.stack([bgr[2:4]] * 4), np.stack([d[2:4] for d in depths]))
    return pipe.dyna.copy(), pipe.label.copy(), pipe.mask.copy(), [[pipe.keypoints(s, t) for t in range(2)] for s in range(4)]


OFF = {}


def switch_off():
    if not OFF:
        pipe = make_pipe(False)
        try:
            OFF["out"] = step(pipe); OFF["sched"] = pipe.last_schedule()
            assert pipe.pieces_batch() == (False, 0, 0) and pipe.device_pieces() == (False, 0, 0)
        finally:
            pipe.close()
    return OFF["out"]


def assert_equal_outputs(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    for s in range(4):
        for t in range(2):
            assert a[3][s][t][0].tobytes() == b[3][s][t][0].tobytes() and np.array_equal(a[3][s][t][1], b[3][s][t][1]), (s, t, "keypoints")


@pytest.mark.parametrize("chunk", [3, None], ids=["chunks_3_1", "default_chunk"])
def test_pipeline_with_the_batched_piece_stage_equals_oracle_and_the_switch_off(chunk):
    bgr, depths, K, refs = case()
    off = switch_off()
    assert all(r[t]["pieces"] >= 1 for r in refs for t in range(2))          # every frame has pieces to cut: (True, 8, 0) below counts them all
    pipe = make_pipe(True, chunk)
    try:
        on = step(pipe)
        assert pipe.last_schedule() == "rounds" == OFF["sched"], pipe.last_schedule()
        assert pipe.pieces_batch() == (True, 8, 0), pipe.pieces_batch()
        assert pipe.device_pieces() == (False, 0, 0)          # the per-tail stage keeps its own count
        assert pipe.rag_batch()[1:] == (8, 0)
    finally:
        pipe.close()
    assert_equal_outputs(off, on)
    orb_ref = O.ORBextractor(*ORB)
    gray = [O.bgr2gray(np.ascontiguousarray(bgr[2 + t]), swap_rb=True) for t in range(2)]
    for s in range(4):
        for t in range(2):
            assert np.array_equal(on[0][s, t], refs[s][t]["dyna"]) and np.array_equal(on[1][s, t], refs[s][t]["label"]), (s, t, "oracle")
            assert np.array_equal(on[2][s, t], refs[s][t]["dilate15"]), (s, t, "mask")
            rk, rdesc = orb_ref.extract(gray[t], refs[s][t]["dilate15"])
            k, d = on[3][s][t]
            assert k.tobytes() == rk.tobytes() and np.array_equal(d, rdesc), (s, t, "ORB")


def test_without_the_batched_rag_stage_the_switch_changes_nothing():
    off = switch_off()
    pipe = make_pipe(True, rag_batch=False)
    try:
        on = step(pipe)
        assert pipe.last_schedule() == "rounds" and pipe.pieces_batch() == (True, 0, 0) and pipe.device_pieces() == (False, 0, 0)
    finally:
        pipe.close()
    assert_equal_outputs(off, on)


def test_a_replayed_step_that_takes_chains_is_untouched_by_the_switch():
    """the first run takes the rounds and the batched stage; the replay of the kept step runs as per-stream chains, where only set_device_pieces decides: same masks,
    labels and fingerprints, and the counters do not move"""
    bgr, depths, K, refs = case()
    pipe = make_pipe(True, 3)
    try:
        pipe.set_chain_max_streams(12)          # (the default: a replay of four streams runs as chains)
        pipe.set_state_hashing(True); pipe.reserve_retained(1)
        start = [pipe.get_state(s) for s in range(4)]
        pipe.retain_next(3)
        pipe.process(np.stack([bgr[2:4]] * 4), np.stack([d[2:4] for d in depths]))
        first = (pipe.dyna.copy(), pipe.label.copy(), pipe.mask.copy(), pipe.state_hashes().copy())
        assert pipe.last_schedule() == "rounds" and pipe.pieces_batch() == (True, 8, 0)
        for s in range(4):
            pipe.set_state(s, start[s])
        pipe.replay(3, [0] * 4, [2] * 4)
        assert "chain" in pipe.last_schedule(), pipe.last_schedule()
        again = (pipe.dyna.copy(), pipe.label.copy(), pipe.mask.copy(), pipe.state_hashes().copy())
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
        assert pipe.pieces_batch() == (True, 8, 0) and pipe.device_pieces() == (False, 0, 0)
    finally:
        pipe.close()


def test_a_ragged_step_completes_its_partial_chunk():
    """streams 0 .. 3 run 2, 1, 2 and 0 frames: round 0 has three frames (one full chunk of 3), round 1 two (a partial chunk, flushed by the round's last frame)"""
    bgr, depths, K, refs = case()
    act = [2, 1, 2, 0]
    outs = {}
    for on in (False, True):
        pipe = make_pipe(on, 3)
        try:
            pipe.set_active_frames(act)
            pipe.process(np.stack([bgr[2:4]] * 4), np.stack([d[2:4] for d in depths]))
            outs[on] = (pipe.dyna.copy(), pipe.label.copy(), pipe.mask.copy())
            if on:
                assert pipe.last_schedule() == "rounds", pipe.last_schedule()
                assert pipe.pieces_batch() == (True, 5, 0), pipe.pieces_batch()
        finally:
            pipe.close()
    for s in range(4):
        for t in range(act[s]):
            for a, b in zip(outs[False], outs[True]):
                assert np.array_equal(a[s, t], b[s, t]), (s, t)
            assert np.array_equal(outs[True][0][s, t], refs[s][t]["dyna"]) and np.array_equal(outs[True][1][s, t], refs[s][t]["label"]), (s, t, "oracle")
