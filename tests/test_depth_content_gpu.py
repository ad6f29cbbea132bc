"""GPU: the whole detector on hostile depth content at the smallest legal frame sizes at which the oracle still forms planes, pieces and a dynamic mask
(test_depth_scene_cpu.py asserts that from the oracle alone): DynaDetect against O.DynaDetect over frames 2 and 3 of a stream -- the second frame takes the
warm-started k-means labels -- on every stage output of test_dyna_gpu.py::test_detect_sequence, and the batched pipeline (B >= 4: the batched CalOccluded
stage) on four streams of four different depth kinds.  Colour comes from SyntheticStream(width, height, seed=3), the depth is rewritten by depth_scene.py."""
import numpy as np
import pytest

import depth_ref as R
import depth_scene as S
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _detect_equals_oracle(bgr, depth, K, what):
    from sindslam_amd.dyna import DynaDetect
    ref = R.oracle_stages(bgr, depth, K)
    gpu = DynaDetect(bgr[1], bgr[0], *K); outs = []
    try:
        for k, t in enumerate((2, 3)):
            gd, gl = gpu.DetectDynaArea(bgr[t], depth[t], t); g = gpu.debug(); r = ref[k]
            for key in R.STAGES:
                a, b = g[key], r[key]
                if key == "centers":
                    a, b = a.view(np.uint32), b.view(np.uint32)
                assert np.array_equal(a, b), (what, t, key, int((a != b).sum()))
            assert g["info"][2] == r["pieces"], (what, t, "pieces", int(g["info"][2]), r["pieces"])
            assert np.array_equal(gd, r["dyna"]), (what, t, "imgDyna", int((gd != r["dyna"]).sum()))
            assert np.array_equal(gl, r["label"]), (what, t, "imgLabel", int((gl != r["label"]).sum()))
            assert np.array_equal(gpu.dilate15(gd), r["dilate15"]), (what, t, "dilate15")
            outs.append((gd, gl))
    finally:
        gpu.close()
    return ref, outs


@pytest.mark.parametrize("w,h,intr,base", S.CONTENT_SIZES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_detector_equals_oracle_on_hostile_depth(w, h, intr, base, kind):
    bgr, depth, K = S.stream_case(w, h, kind, intr, base)
    ref, _ = _detect_equals_oracle(bgr, depth, K, (w, h, kind))
    if kind in ("plain", "saturated", "steps", "border"):                     # (the full conditions: test_depth_scene_cpu.py)
        assert all(o["pieces"] >= 8 and o["occ2"].any() and (o["dyna"] == 255).any() for o in ref)


@pytest.mark.parametrize("w,h", S.SMALL_PLAIN)
def test_detector_equals_oracle_at_the_smallest_sizes(w, h):
    """64 x 64 and 128 x 72: no plane and nothing dynamic is found, but what is computed equals the oracle"""
    bgr, depth, K = S.stream_case(w, h, "plain")
    _detect_equals_oracle(bgr, depth, K, (w, h, "plain"))


@pytest.mark.parametrize("w,h", [(192, 144), (192, 136)])
def test_batched_pipeline_on_four_different_depth_kinds(w, h):
    """Pipeline(4, 2): the CalOccluded front and the depth normalisation of the four frames of a round run in ONE launch each, with per-frame maxima -- on streams
    that differ (plain / an all-zero frame first / saturated / lowrange) a maximum read from a neighbour's slot changes the result.  Every stream equals the
    single-frame DynaDetect of the same stream and the oracle: masks, labels, key points and descriptors."""
    from sindslam_amd.pipeline import Pipeline
    bgr, plain, K = S.stream_case(w, h, "plain")
    zero_first = plain.copy(); zero_first[2] = 0
    depths = [plain, zero_first, S.stream_case(w, h, "saturated")[1], S.stream_case(w, h, "lowrange")[1]]
    assert sorted(int(d[2].max()) for d in depths)[:2] == [0, 510] and int(depths[2][2].max()) == 65535 and 510 < int(plain[2].max()) < 65535
    singles = [_detect_equals_oracle(bgr, d, K, (w, h, "stream", s)) for s, d in enumerate(depths)]
    orb = (1000, 1.2, 8, 15, 5); orb_ref = O.ORBextractor(*orb)
    pipe = Pipeline(4, 2, w, h, *K, *orb, orb_gray_rgb_order=1)
    try:
        for s in range(4):
            pipe.prime(s, bgr[1], bgr[0])
        pipe.process(np.stack([bgr[2:4]] * 4), np.stack([d[2:4] for d in depths]))
        gray = [O.bgr2gray(np.ascontiguousarray(bgr[2 + t]), swap_rb=True) for t in range(2)]
        nk = 0
        for s in range(4):
            ref, outs = singles[s]
            for t in range(2):
                assert np.array_equal(pipe.dyna[s, t], outs[t][0]) and np.array_equal(pipe.label[s, t], outs[t][1]), (s, t, "single-frame DynaDetect")
                assert np.array_equal(pipe.dyna[s, t], ref[t]["dyna"]) and np.array_equal(pipe.label[s, t], ref[t]["label"]), (s, t, "oracle")
                assert np.array_equal(pipe.mask[s, t], ref[t]["dilate15"]), (s, t, "mask")
                rk, rdesc = orb_ref.extract(gray[t], ref[t]["dilate15"])
                k, d = pipe.keypoints(s, t)
                assert k.tobytes() == rk.tobytes() and np.array_equal(d, rdesc), (s, t, "ORB", len(k), len(rk))
                nk += len(k)
        assert nk > 0
        assert not singles[1][0][0]["dyna"].any() and singles[1][0][1]["dyna"].any()              # the all-zero frame gives an empty mask, the stream recovers on the next
    finally:
        pipe.close()
