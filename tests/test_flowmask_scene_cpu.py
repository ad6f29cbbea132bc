"""CPU: the numpy restatement of the flow-mask stage (tests/flowmask_ref.py) against the oracle's block (oracle_lib.flow_masks, Otsu, Triangle) on every scene of
tests/flowmask_scene.py and on real stream frames; every scene's stated property; and the branch record: which comparisons of the clamps the scenes take."""
import numpy as np
import pytest

import flowmask_ref as R
import flowmask_scene as S
import oracle_lib as O
from sindslam_amd.synth import TUM3


def _same_as_oracle(r, o, what):
    assert np.array_equal(r["hist"], o["hist"]), what
    assert np.float32(r["maxError"]).view(np.int32) == np.float32(o["maxError"]).view(np.int32), (what, r["maxError"], o["maxError"])
    for k in ("otsu", "triangle", "lo", "hi"):
        assert np.float32(r[k]).view(np.int32) == np.float32(o[k]).view(np.int32), (what, k, r[k], o[k])
    assert np.array_equal(r["mag_u8"], o["mag_u8"]), what
    assert np.array_equal(r["mask_low"], o["mask_low"]) and np.array_equal(r["mask_high"], o["mask_high"]), what


@pytest.mark.parametrize("size", S.SIZES + [(640, 480)])
def test_reference_equals_the_oracle_on_every_field(size):
    W, H = size
    scenes = S.fields(W, H) if size in S.SIZES else S.few_fields(W, H)
    assert len(scenes) >= 10
    for s in scenes:
        _same_as_oracle(s.ref(), O.flow_masks(s.u, s.v, s.Hm), (s.name, size))


@pytest.mark.parametrize("size", S.BLOCK_SIZES)
def test_reference_equals_the_oracle_on_every_block(size):
    """the rule and shape blocks and the ten kinds of histogram: Otsu and Triangle against the oracle's"""
    W, H = size; N = W * H
    for s in S.blocks(W, H):
        r = s.ref()
        assert s.hist.sum() == N and r["otsu"] == np.float32(O.otsu(s.hist)) and r["triangle"] == np.float32(O.triangle(s.hist)), (s.name, size)
    kinds = S.hist_kinds(np.random.default_rng(N), 40 if N > 640 * 480 else 100, N)
    otsu = R.otsu(kinds[:, :256], N)[0]
    for k in range(len(kinds)):
        h = np.ascontiguousarray(kinds[k, :256])
        assert otsu[k] == O.otsu(h) and R.triangle(h) == O.triangle(h), (k, size)


@pytest.mark.parametrize("size", S.BLOCK_SIZES)
def test_every_scene_has_the_property_it_was_built_for(size):
    W, H = size
    scenes = S.blocks(W, H) + (S.fields(W, H) if size in S.SIZES else S.few_fields(W, H) if size == (640, 480) else [])
    for s in scenes:
        assert s.holds(s.ref()), (s.name, size, s.prop)


@pytest.mark.parametrize("size", S.BLOCK_SIZES)
def test_scenes_take_every_comparison_both_ways(size):
    """from the reference's own record: every comparison of the clamps (flow_mask.hip: the thred1 < thred2 branch, four clamp comparisons and the arm of the maximum in
    each branch, the count rule) is taken both ways, the tie thred1 == thred2 is there, and the count sits on N / 2 and on N / 2 + 1"""
    W, H = size; N = W * H
    seen = {k: set() for k in R.COMPARISONS}; tie = False; counts = set()
    for s in S.blocks(W, H):
        r = s.ref(); rec = r["rec"]
        for k in R.COMPARISONS:
            if k in rec:
                seen[k].add(rec[k])
        tie |= bool(r["otsu"] == r["triangle"])
        if "A.count" in rec:
            counts.add(rec["A.count"])
    assert all(v == {True, False} for v in seen.values()), {k: v for k, v in seen.items() if v != {True, False}}
    assert tie and N // 2 in counts and N // 2 + 1 in counts
    if size in S.SIZES:                                   # the fields take them too, but for the rules a frame of that size cannot reach with a pixel in bin 255
        seen_f = {k: set() for k in R.COMPARISONS}
        for s in S.fields(W, H):
            for k in R.COMPARISONS:
                if k in s.ref()["rec"]:
                    seen_f[k].add(s.ref()["rec"][k])
        missing = [k for k, v in seen_f.items() if v != {True, False}]
        assert missing == [], missing


def test_reference_reproduces_the_oracle_detector_on_stream_frames(frames):
    """two real frames: the reference, fed the oracle's own flow_full and H, gives the oracle's histogram, thresholds and masks; the branch each frame takes is recorded"""
    bgr, depth = frames
    K = (TUM3["fx"], TUM3["fy"], TUM3["cx"], TUM3["cy"], TUM3["depth_factor"])
    det = O.DynaDetect(bgr[1], bgr[0], *K)
    branches = []
    for t in (2, 3):
        det.detect(bgr[t], depth[t]); d = det.debug()
        r = R.stage(d["flow_full"][..., 0], d["flow_full"][..., 1], d["H"])
        assert np.array_equal(r["hist"], d["hist"])
        got = np.array([r["maxError"], r["otsu"], r["triangle"], r["lo"], r["hi"]], np.float32)
        assert np.array_equal(got.view(np.int32), d["thr"].view(np.int32)), (got, d["thr"])
        assert np.array_equal(r["mag_u8"], d["mag_u8"]) and np.array_equal(r["mask_low"], d["mask_low"]) and np.array_equal(r["mask_high"], d["mask_high"])
        o = O.flow_masks(d["flow_full"][..., 0], d["flow_full"][..., 1], d["H"])
        _same_as_oracle(r, o, t)
        branches.append(bool(r["rec"]["otsu<tri"]))
    assert branches == [False, False]                     # a heavy head: Triangle lies below Otsu, both frames take the else branch
