"""GPU: the GATHERED second DeepFlow pass of the batched pipeline (DynaFront::dense_flow without `speculate`: the flagged pairs of a slice are collected into a
batch of their own, solved at that batch size on the slice's flow engine, scattered back to their slots, and the refinement picks frame n-1 or n-2 per pair) on
steps that MIX large-motion and calm pairs.  Streams and their flags come from motion_scene.py; test_motion_scene_cpu.py asserts, from the oracle alone, that
every step here holds both kinds, that flagged[k] != k occurs, and that the flagged frames' imgDyna changes with the flow path.  For every stream and frame:
Pipeline.large_motion() is the oracle's flag, imgDyna / imgLabel / the dilated mask / ORB keypoints and descriptors are the oracle's."""
import numpy as np
import pytest

import motion_scene as M

pytestmark = pytest.mark.gpu


def _pipeline(name, **kw):
    from sindslam_amd.pipeline import Pipeline
    w, h, S, T, slices, streams = M.CONFIGS[name]
    pipe = Pipeline(S, T, w, h, *M.intrinsics(w), *M.ORB, orb_gray_rgb_order=1, flow_slices=slices, **kw)
    data = [M.stream(w, h, s) for s in streams]
    for s in range(S):
        pipe.prime(s, data[s][0][1], data[s][0][0])
    return pipe, data


def _step(pipe, data, step):
    lo = 2 + step * pipe.T
    pipe.process(np.stack([d[0][lo:lo + pipe.T] for d in data]), np.stack([d[1][lo:lo + pipe.T] for d in data]))
    return lo


def _outputs(pipe):
    return pipe.dyna.copy(), pipe.label.copy(), pipe.mask.copy(), pipe.nkp.copy(), pipe.kps.copy(), pipe.desc.copy(), pipe.large_motion()


def _check_frame(pipe, name, s, t, f, tag):
    w, h, _, _, _, streams = M.CONFIGS[name]
    r = M.oracle_run(w, h, streams[s])[f]; what = (name, tag, "stream", s, streams[s], "frame", f)
    assert np.array_equal(pipe.dyna[s, t], r["dyna"]), (what, "imgDyna", int((pipe.dyna[s, t] != r["dyna"]).sum()))
    assert np.array_equal(pipe.label[s, t], r["label"]), (what, "imgLabel", int((pipe.label[s, t] != r["label"]).sum()))
    assert np.array_equal(pipe.mask[s, t], r["mask"]), (what, "dilate15")
    k, d = pipe.keypoints(s, t)
    assert k.tobytes() == r["keypoints"].tobytes() and np.array_equal(d, r["descriptors"]), (what, "ORB", len(k), len(r["keypoints"]))
    return len(k)


def _check_flags(pipe, name, lo, tag):
    w, h, S, T, _, streams = M.CONFIGS[name]
    want = np.array([[M.oracle_run(w, h, streams[s])[lo + t]["flag"] for t in range(T)] for s in range(S)], np.int32)
    got = pipe.large_motion()
    assert got.shape == (S, T) and got.dtype == np.int32 and np.array_equal(got, want), (name, tag, "large_motion", got.tolist(), want.tolist())
    assert want.ravel().tolist() == M.config_flags(name)[(lo - 2) // T]              # ... and the oracle's flag is the recorded one: the step is mixed
    return want


@pytest.mark.parametrize("name", ["one_slice", "slices_clean", "slices_mixed", "three_slices", "walkers"])
def test_mixed_steps_equal_the_oracle(name):
    pipe, data = _pipeline(name)
    try:
        nk = 0
        for step in range(M.STEPS):
            lo = _step(pipe, data, step)
            assert pipe.stats()["sor_slices"] == M.CONFIGS[name][4]
            _check_flags(pipe, name, lo, step)
            for s in range(pipe.S):
                for t in range(pipe.T):
                    nk += _check_frame(pipe, name, s, t, lo + t, step)
        assert nk > 0
    finally:
        pipe.close()


def test_one_pair_gathered_equals_the_oracle_and_the_speculative_detector():
    """Pipeline(1, 1): B = B2 = 1 on the gathered path, against the oracle and, byte for byte, against DynaDetect, which solves both passes in one batch of two"""
    from sindslam_amd.dyna import DynaDetect
    name = "one_one"; pipe, data = _pipeline(name); bgr, depth = data[0]
    dd = DynaDetect(bgr[1], bgr[0], *M.intrinsics(M.CONFIGS[name][0]))
    try:
        flags = []
        for step in range(M.STEPS):
            lo = _step(pipe, data, step)
            flags.append(int(_check_flags(pipe, name, lo, step)[0, 0]))
            _check_frame(pipe, name, 0, 0, lo, step)
            gd, gl = dd.DetectDynaArea(bgr[lo], depth[lo], lo)
            assert int(dd.debug()["info"][0]) == flags[-1]
            assert pipe.dyna[0, 0].tobytes() == gd.tobytes() and pipe.label[0, 0].tobytes() == gl.tobytes() and pipe.mask[0, 0].tobytes() == dd.dilate15(gd).tobytes(), lo
        assert flags == [1, 0]
    finally:
        dd.close(); pipe.close()


def test_ragged_step_on_a_mixed_batch():
    """a full step, then set_active_frames([2, 1, 0, 2]) as rounds (set_chain_max_streams(0)): the flags cover every pair (they depend on the frames alone), the
    frames whose tails ran equal the oracle, the others keep the previous step's outputs"""
    name = M.RAGGED; pipe, data = _pipeline(name)
    try:
        pipe.set_chain_max_streams(0)
        lo = _step(pipe, data, 0); _check_flags(pipe, name, lo, "full")
        for s in range(pipe.S):
            for t in range(pipe.T):
                _check_frame(pipe, name, s, t, lo + t, "full")
        keep = pipe.dyna.copy(); act = [2, 1, 0, 2]
        pipe.set_active_frames(np.array(act, np.int32))
        lo = _step(pipe, data, 1); _check_flags(pipe, name, lo, "ragged")
        for s in range(pipe.S):
            for t in range(pipe.T):
                if t < act[s]:
                    _check_frame(pipe, name, s, t, lo + t, "ragged")
                else:
                    assert np.array_equal(pipe.dyna[s, t], keep[s, t]), (s, t)
    finally:
        pipe.close()


def test_flow_mask_and_rag_batching_do_not_change_a_mixed_step():
    """flow-mask and RAG stages batched per k-means round (two pool workers for four streams: non-split rounds) or per frame: the same outputs, equal to the oracle"""
    name = M.BATCH_SWITCHES; got = {}
    for on in (True, False):
        pipe, data = _pipeline(name, host_threads=2)
        try:
            pipe.set_flow_mask_batch(on); pipe.set_rag_batch(on); steps = []
            for step in range(M.STEPS):
                lo = _step(pipe, data, step); _check_flags(pipe, name, lo, (on, step)); steps.append(_outputs(pipe))
                if on:
                    for s in range(pipe.S):
                        for t in range(pipe.T):
                            _check_frame(pipe, name, s, t, lo + t, (on, step))
            assert pipe.flow_mask_batch() == (on, pipe.S * pipe.T * M.STEPS if on else 0)
            assert pipe.rag_batch()[0] == on and (on or pipe.rag_batch()[1] == 0)
            got[on] = steps
        finally:
            pipe.close()
    for step in range(M.STEPS):
        a, b = got[True][step], got[False][step]
        for i in (0, 1, 2, 3, 6):
            assert np.array_equal(a[i], b[i]), (step, i)
        for k in range(len(a[3])):
            n = a[3][k]; assert a[4][k, :n].tobytes() == b[4][k, :n].tobytes() and np.array_equal(a[5][k, :n], b[5][k, :n]), (step, k)


def test_pipeline_group_concatenates_the_flags():
    """PipelineGroup(2, ...) over the one-slice configuration: the members' flags in stream order, as state_hashes are"""
    from sindslam_amd.pipeline import PipelineGroup
    name = "one_slice"; w, h, S, T, _, streams = M.CONFIGS[name]
    grp = PipelineGroup(2, S, T, w, h, *M.intrinsics(w), *M.ORB, orb_gray_rgb_order=1)
    try:
        data = [M.stream(w, h, s) for s in streams]
        for s in range(S):
            grp.prime(s, data[s][0][1], data[s][0][0])
        grp.process(np.stack([d[0][2:2 + T] for d in data]), np.stack([d[1][2:2 + T] for d in data]))
        _check_flags(grp, name, 2, "group")
        for s in range(S):
            for t in range(T):
                _check_frame(grp, name, s, t, 2 + t, "group")
    finally:
        grp.close()


def test_getter_before_the_first_step_is_an_error():
    from sindslam_amd._lib import SindError
    pipe, _ = _pipeline("one_one")
    try:
        with pytest.raises(SindError, match="no step has finished"):
            pipe.large_motion()
    finally:
        pipe.close()


@pytest.mark.timeout(600)
def test_in_order_driver_across_calm_fast_and_static_chunks():
    """process_sequence_exact over 24 frames (eight each of a calm, a fast and a standing camera, a block moving throughout) in three steps of eight: every frame
    equals the oracle's in-order loop on imgDyna, imgLabel and the dilated mask.  The oracle's flags change inside two of the chunks and across a seam
    (test_motion_scene_cpu.py)."""
    import oracle_lib as O
    from sindslam_amd.sequence import process_sequence_exact
    bgr, depth = M.seq_frames(); intr = M.seq_intr(); n = len(bgr)
    ref = O.sequence_run(bgr, depth, intr, threads=8, want_orb=False)
    got = process_sequence_exact(np.array(bgr), np.array(depth), intr, frames_per_step=M.SEQ_STEP, nfeatures=M.ORB[0], want_keypoints=False)
    assert got["owned"] == list(range(1, n))
    dyn = 0
    for f in range(1, n):
        assert np.array_equal(got["dyna"][f], ref["dyna"][f]), (f, "imgDyna", int((got["dyna"][f] != ref["dyna"][f]).sum()))
        assert np.array_equal(got["label"][f], ref["label"][f]), (f, "imgLabel")
        assert np.array_equal(got["mask"][f], ref["mask"][f]), (f, "dilate15")
        dyn += int((ref["dyna"][f] == 255).any())
    assert dyn > n // 2
