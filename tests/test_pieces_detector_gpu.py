"""GPU: the detector and the batched pipeline with SegAndMerge's piece extraction switched to the GPU (set_device_pieces), against the oracle and against the same
run with the switch off: two frames each at 192 x 136, 192 x 144, 256 x 192 and 320 x 240 on the plain, stepped and speckled depth of depth_scene.py, and
Pipeline(4, 2) on four depth kinds with the region-adjacency stage batched per round and per frame.  device_pieces() must report every frame on the device and none fallen back: an equal result
through a silent fallback would prove nothing."""
import numpy as np
import pytest

import depth_ref as R
import depth_scene as S
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,intr,base", S.CONTENT_SIZES)
@pytest.mark.parametrize("kind", ["plain", "steps", "speckle"])
def test_detector_with_device_pieces_equals_oracle(w, h, intr, base, kind):
    from sindslam_amd.dyna import DynaDetect
    bgr, depth, K = S.stream_case(w, h, kind, intr, base)
    ref = R.oracle_stages(bgr, depth, K)
    gpu = DynaDetect(bgr[1], bgr[0], *K)
    try:
        assert gpu.device_pieces() == (False, 0, 0)
        gpu.set_device_pieces(True)
        for k, t in enumerate((2, 3)):
            gd, gl = gpu.DetectDynaArea(bgr[t], depth[t], t); r = ref[k]
            assert np.array_equal(gl, r["label"]), (t, "imgLabel", int((gl != r["label"]).sum()))
            assert np.array_equal(gd, r["dyna"]), (t, "imgDyna", int((gd != r["dyna"]).sum()))
            assert np.array_equal(gpu.dilate15(gd), r["dilate15"]), (t, "dilate15")
        assert gpu.device_pieces() == (True, 2, 0)
        assert any(o["pieces"] >= 2 for o in ref)
    finally:
        gpu.close()


@pytest.mark.parametrize("rag_batch", [True, False], ids=["rag_batched", "rag_per_frame"])
def test_pipeline_with_device_pieces_equals_oracle_and_the_switch_off(rag_batch):
    from sindslam_amd.pipeline import Pipeline
    w, h = 192, 144
    bgr, plain, K = S.stream_case(w, h, "plain")
    depths = [plain, S.stream_case(w, h, "steps")[1], S.stream_case(w, h, "speckle")[1], S.stream_case(w, h, "lowrange")[1]]
    refs = [R.oracle_stages(bgr, d, K) for d in depths]
    orb = (1000, 1.2, 8, 15, 5); orb_ref = O.ORBextractor(*orb)
    gray = [O.bgr2gray(np.ascontiguousarray(bgr[2 + t]), swap_rb=True) for t in range(2)]
    outs = {}
    for on in (False, True):
        pipe = Pipeline(4, 2, w, h, *K, *orb, orb_gray_rgb_order=1)
        try:
            pipe.set_chain_max_streams(0); pipe.set_rag_batch(rag_batch)
            pipe.set_device_pieces(on)
            for s in range(4):
                pipe.prime(s, bgr[1], bgr[0])
            pipe.process(np.stack([bgr[2:4]] * 4), np.stack([d[2:4] for d in depths]))
            outs[on] = (pipe.dyna.copy(), pipe.label.copy(), pipe.mask.copy(), [[pipe.keypoints(s, t) for t in range(2)] for s in range(4)])
            assert pipe.device_pieces() == ((True, 8, 0) if on else (False, 0, 0))
        finally:
            pipe.close()
    for a, b in zip(outs[False][:3], outs[True][:3]):
        assert np.array_equal(a, b)
    for s in range(4):
        for t in range(2):
            assert np.array_equal(outs[True][0][s, t], refs[s][t]["dyna"]) and np.array_equal(outs[True][1][s, t], refs[s][t]["label"]), (s, t, "oracle")
            assert np.array_equal(outs[True][2][s, t], refs[s][t]["dilate15"]), (s, t, "mask")
            rk, rdesc = orb_ref.extract(gray[t], refs[s][t]["dilate15"])
            for side in (False, True):
                k, d = outs[side][3][s][t]
                assert k.tobytes() == rk.tobytes() and np.array_equal(d, rdesc), (s, t, side, "ORB")


def test_a_retained_step_replayed_as_chains_with_device_pieces_equals_its_first_run():
    """Pipeline(4, 2) with the switch on: the step is kept, the states are put back and its tails run again over all frames -- as per-stream chains (a replay of four
    streams), where the first run took batched rounds.  Same masks, labels, fingerprints; equal to the oracle; every frame of both runs on the device"""
    from sindslam_amd.pipeline import Pipeline
    w, h = 192, 144
    bgr, plain, K = S.stream_case(w, h, "plain")
    depths = [plain, S.stream_case(w, h, "steps")[1], S.stream_case(w, h, "speckle")[1], S.stream_case(w, h, "lowrange")[1]]
    refs = [R.oracle_stages(bgr, d, K) for d in depths]
    pipe = Pipeline(4, 2, w, h, *K, 1000, 1.2, 8, 15, 5, orb_gray_rgb_order=1)
    try:
        pipe.set_device_pieces(True); pipe.set_state_hashing(True); pipe.reserve_retained(1)
        for s in range(4):
            pipe.prime(s, bgr[1], bgr[0])
        start = [pipe.get_state(s) for s in range(4)]
        pipe.retain_next(3)
        pipe.process(np.stack([bgr[2:4]] * 4), np.stack([d[2:4] for d in depths]))
        first = (pipe.dyna.copy(), pipe.label.copy(), pipe.mask.copy(), pipe.state_hashes().copy()); sched = pipe.last_schedule()
        assert "chain" not in sched and pipe.device_pieces() == (True, 8, 0)
        for s in range(4):
            pipe.set_state(s, start[s])
        pipe.replay(3, [0] * 4, [2] * 4)
        assert "chain" in pipe.last_schedule(), pipe.last_schedule()
        again = (pipe.dyna.copy(), pipe.label.copy(), pipe.mask.copy(), pipe.state_hashes().copy())
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
        assert pipe.device_pieces() == (True, 16, 0)
        for s in range(4):
            for t in range(2):
                assert np.array_equal(again[0][s, t], refs[s][t]["dyna"]) and np.array_equal(again[1][s, t], refs[s][t]["label"]), (s, t)
    finally:
        pipe.close()
