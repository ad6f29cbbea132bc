"""GPU parity of the batched flow-mask stage (FlowMaskBatch: one frame of every stream of a k-means group in four launches, masks bit-packed) against the
per-frame stage it replaces in the non-split rounds: the kernels through the debug entry, and whole pipeline steps with the switch on and off."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from sindslam_amd._lib import check, lib, ptr
from sindslam_amd.synth import TUM3

pytestmark = pytest.mark.gpu

K = (TUM3["fx"], TUM3["fy"], TUM3["cx"], TUM3["cy"], TUM3["depth_factor"])


def _stage_frames(W, H, count):
    """count frames of (U, V, homography).  A: smooth flow + noise under a perspective homography; Z: identity and zero flow (maximal residual 0: 255 / 0 in the
    normalisation); X: one huge residual, every other pixel in bin 0; B: another ordinary frame; the last frame of a batch of 3 or 5 repeats A."""
    rng = np.random.default_rng(1000 * W + H)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)

    def ordinary(k):
        u = (0.8 * np.sin(xx / (7.0 + k)) + rng.normal(0, 0.6, (H, W))).astype(np.float32); v = (0.5 * np.cos(yy / (5.0 + k)) + rng.normal(0, 0.6, (H, W))).astype(np.float32)
        u[H // 3: H // 3 + max(2, H // 4), W // 4: W // 4 + W // 5] += 6.0 + k                                  # a moving block: a second mode for Otsu / Triangle
        hm = np.array([1.0 + 1e-3 * (k + 1), 2e-4, 0.3 * (k + 1), -3e-4, 1.0 - 2e-3, -0.2, 1e-6 * (k + 1), -2e-6, 1.0])
        return u, v, hm
    eye = np.eye(3).ravel()
    A = ordinary(0); B = ordinary(1)
    Z = (np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), eye.copy())
    xu = np.zeros((H, W), np.float32); xu[H // 2, W // 2 + 1] = 3.0e6
    X = (xu, np.zeros((H, W), np.float32), eye.copy())
    order = {1: [A], 3: [A, Z, A], 5: [A, Z, X, B, A]}[count]
    return (np.ascontiguousarray(np.stack([f[0] for f in order])), np.ascontiguousarray(np.stack([f[1] for f in order])),
            np.ascontiguousarray(np.stack([f[2] for f in order])))


@pytest.mark.parametrize("count", [1, 3, 5])
@pytest.mark.parametrize("size", [(64, 8), (128, 24), (640, 480)])
def test_batched_stage_equals_per_frame_kernels(size, count):
    """masks, histogram, maximum and the four thresholds of every frame: byte-equal between the four batched launches and the per-frame kernels
    (64 x 8: one word per row, two row groups of the residual kernel; 640 x 480: the production size, many blocks per frame)"""
    W, H = size
    u, v, hm = _stage_frames(W, H, count)
    n = count; npx = W * H
    lb = np.full((n, npx), 7, np.uint8); hb = np.full((n, npx), 7, np.uint8); rb = np.full((n, 261), -1, np.int32)
    lf = np.full((n, npx), 9, np.uint8); hf = np.full((n, npx), 9, np.uint8); rf = np.full((n, 261), -2, np.int32)
    check(lib().sind_debug_flow_masks_batch(ptr(u), ptr(v), ptr(hm), n, W, H, 0, ptr(lb), ptr(hb), ptr(rb), ptr(lf), ptr(hf), ptr(rf)), "sind_debug_flow_masks_batch")
    for i in range(n):
        assert rb[i].tobytes() == rf[i].tobytes(), (i, rb[i, 256:], rf[i, 256:])        # histogram, maximum, lo / hi / otsu / triangle
        assert np.array_equal(lb[i], lf[i]) and np.array_equal(hb[i], hf[i]), i
        assert rf[i, :256].sum() == npx and set(np.unique(lf[i])) <= {0, 128} and set(np.unique(hf[i])) <= {0, 255}
    if count >= 3:                                                                     # the repeated frame: the same bytes twice
        assert rb[0].tobytes() == rb[n - 1].tobytes() and np.array_equal(lb[0], lb[n - 1]) and np.array_equal(hb[0], hb[n - 1])
        assert rb[1, 256] == 0                                                         # identity and zero flow: maximal residual 0.0
    if count == 5:
        assert rb[2, 0] == npx - 1 and rb[2, 255] == 1                                 # one huge residual: everything else in bin 0
    assert 0 < (lb[0] != 0).sum() < npx                                                # an ordinary frame has a real mask


def _streams(frames, S):
    bgr, depth = frames
    vb = [bgr, bgr[:, ::-1], bgr[:, :, ::-1], bgr[:, ::-1, ::-1]]; vd = [depth, depth[:, ::-1], depth[:, :, ::-1], depth[:, ::-1, ::-1]]
    return np.stack([np.ascontiguousarray(vb[s]) for s in range(S)]), np.stack([np.ascontiguousarray(vd[s]) for s in range(S)])


def _outputs(p):
    return p.dyna.copy(), p.label.copy(), p.mask.copy(), p.nkp.copy(), p.kps.copy(), p.desc.copy()


def _assert_same(a, b, what):
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y), what
    for k in range(len(a[3])):
        n = a[3][k]; assert a[4][k, :n].tobytes() == b[4][k, :n].tobytes() and np.array_equal(a[5][k, :n], b[5][k, :n]), (what, k)


def test_pipeline_batch_on_equals_off(frames):
    """three streams on two pool workers (more streams than workers: non-split rounds), two steps: every output of the batched flow-mask stage equals the
    per-frame stage's, all 12 frames come from batches, and two streams of the first step equal the oracle"""
    from sindslam_amd.pipeline import Pipeline
    S, T = 3, 2
    sb, sd = _streams(frames, S)
    got = {}
    for on in (True, False):
        pipe = Pipeline(S, T, 640, 480, *K, 1500, 1.2, 8, 15, 5, orb_gray_rgb_order=1, host_threads=2)
        assert pipe.flow_mask_batch() == (True, 0)                                     # on by default
        pipe.set_flow_mask_batch(on)
        for s in range(S):
            pipe.prime(s, sb[s, 1], sb[s, 0])
        steps = []
        for step in range(2):
            lo = 2 + step * T
            pipe.process(sb[:, lo:lo + T], sd[:, lo:lo + T]); steps.append(_outputs(pipe))
        assert pipe.flow_mask_batch() == (on, 12 if on else 0)
        got[on] = steps; pipe.close()
    for step in range(2):
        _assert_same(got[True][step], got[False][step], step)
    assert (got[True][1][1] > 0).any()
    dyna, label, mask, nkp, kps, desc = got[True][0]
    orb_ref = O.ORBextractor(1500, 1.2, 8, 15, 5)
    for s in (0, 2):
        ref = O.DynaDetect(np.ascontiguousarray(sb[s, 1]), np.ascontiguousarray(sb[s, 0]), *K)
        for t in range(T):
            rd, rl = ref.detect(np.ascontiguousarray(sb[s, 2 + t]), np.ascontiguousarray(sd[s, 2 + t]))
            gd = dyna[s, t]
            u = np.logical_or(gd == 255, rd == 255).sum()
            iou = 1.0 if u == 0 else np.logical_and(gd == 255, rd == 255).sum() / u
            assert iou >= 0.99, (s, t, iou)
            assert np.array_equal(mask[s, t], O.dilate15(gd))
            rk, rdesc = orb_ref.extract(O.bgr2gray(np.ascontiguousarray(sb[s, 2 + t]), swap_rb=True), mask[s, t])
            k = s * T + t; n = nkp[k]
            assert kps[k, :n].tobytes() == rk.tobytes() and np.array_equal(desc[k, :n], rdesc), (s, t)


def test_ragged_step_batch_on_equals_off(frames):
    """a ragged step as rounds (no per-stream chains): streams with 2, 1, 0 and 2 active frames -- a round's batch holds only the streams that have a frame in it"""
    from sindslam_amd.pipeline import Pipeline
    S, T = 4, 2
    sb, sd = _streams(frames, S)
    got = {}
    for on in (True, False):
        pipe = Pipeline(S, T, 640, 480, *K, 1500, 1.2, 8, 15, 5, orb_gray_rgb_order=1, host_threads=2)
        pipe.set_chain_max_streams(0); pipe.set_state_hashing(True); pipe.set_flow_mask_batch(on)
        for s in range(S):
            pipe.prime(s, sb[s, 1], sb[s, 0])
        pipe.set_active_frames(np.array([2, 1, 0, 2], np.int32))
        pipe.process(sb[:, 2:2 + T], sd[:, 2:2 + T])
        assert pipe.flow_mask_batch() == (on, 5 if on else 0)
        got[on] = (_outputs(pipe), pipe.state_hashes(), [pipe.get_state(s) for s in range(S)]); pipe.close()
    _assert_same(got[True][0], got[False][0], "ragged")
    h = got[True][1]
    assert np.array_equal(h, got[False][1]) and (h[0] != 0).any(axis=1).all() and (h[1, 0] != 0).any() and (h[1, 1] == 0).all() and (h[2] == 0).all()
    for s in range(S):
        assert np.array_equal(got[True][2][s], got[False][2][s]), s
