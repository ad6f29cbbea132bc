"""GPU parity of the batched region-adjacency (RAG) stage of SegAndMerge (RagBatch: a chunk of one k-means group's frames in two launches) against the per-frame
stage it replaces in the non-split rounds: the kernels through the debug entry (against the per-frame kernels and against numpy counts), and whole pipeline
steps with the switch on and off."""
import ctypes as C

import numpy as np
import pytest

from sindslam_amd._lib import check, lib, ptr
from sindslam_amd.synth import TUM3

pytestmark = pytest.mark.gpu

K = (TUM3["fx"], TUM3["fy"], TUM3["cx"], TUM3["cy"], TUM3["depth_factor"])
PIECES = {1: [1], 3: [2, 64, 1], 5: [3, 65, 64, 1, 3]}


def _pack(bits):
    """bool [..., H, W] -> u64 [..., H, W / 64], bit i of word k = pixel 64 k + i"""
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view(np.uint64)


def _unpack(words, W):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[..., :W].astype(bool)


def _frame(rng, W, H, Cn, kind):
    """piece planes, connection planes (bool [Cn][H][W]), occ2 and depthN (u8 [H][W]) of one frame.  kind 0: pieces 0 and 1 identical (when there are two), depthN with
    255 in it; 1: no connection plane set, occ2 all set; 2: occ2 all clear; 3: ordinary"""
    img = np.zeros((Cn, H, W), bool); lj = np.zeros((Cn, H, W), bool)
    for c in range(Cn):
        w = int(rng.integers(2, max(3, W // 2))); h = int(rng.integers(1, max(2, H // 2)))
        x = int(rng.integers(0, W - w + 1)); y = int(rng.integers(0, H - h + 1))
        img[c, y:y + h, x:x + w] = True
        img[c] |= rng.random((H, W)) < 0.01                                        # stray pixels: rows and words the rectangle does not touch
        if kind != 1 and c % 3 != 1:                                               # (every third piece has no connection area)
            lj[c, max(0, y - 1):y + h + 1, max(0, x - 2):x + 2] = True; lj[c] |= rng.random((H, W)) < 0.02
    if kind == 0 and Cn >= 2:
        img[1] = img[0]
    occ2 = (rng.random((H, W)) < 0.3).astype(np.uint8) * 255
    if kind == 1: occ2[:] = 255
    if kind == 2: occ2[:] = 0
    depth_n = rng.integers(0, 255, (H, W)).astype(np.uint8)
    if kind == 0:
        depth_n[rng.random((H, W)) < 0.2] = 255; depth_n[0, 0] = 255
    return img, lj, occ2, depth_n


def _batch(W, H, count):
    rng = np.random.default_rng(77 * W + H + count)
    fr = [_frame(rng, W, H, Cn, i if i < 3 else 3) for i, Cn in enumerate(PIECES[count])]
    if count == 5:
        fr[4] = fr[0]                                                              # the repeated frame
    return fr


def _expected(fr, W, H):
    """the five outputs of one frame from numpy counts; the dilated planes come from sind_debug_dilate_planes"""
    img, lj, occ2, dn = fr; Cn = img.shape[0]
    words = _pack(img); dil_w = np.zeros_like(words)
    check(lib().sind_debug_dilate_planes(ptr(words), Cn, W, H, 7, 0, ptr(dil_w)), "sind_debug_dilate_planes")
    dil = _unpack(dil_w, W).reshape(Cn, -1).astype(np.float64)
    upper = np.triu(np.ones((Cn, Cn), bool), 1)
    ov = np.where(upper, dil @ dil.T, 0).astype(np.int64)
    dpl = dil * (occ2.reshape(-1) != 0)
    ovp = np.where(upper, dpl @ dil.T, 0).astype(np.int64)
    ljf = lj.reshape(Cn, -1).astype(np.float64)
    ljo = np.where(upper, ljf @ ljf.T, 0).astype(np.int64)
    lja = lj.reshape(Cn, -1).sum(axis=1).astype(np.int64)
    hist = np.zeros((Cn, 256), np.int64)
    for c in range(Cn):
        hist[c, :255] = np.bincount(dn[img[c]], minlength=256)[:255]               # value 255 is dropped
    return np.concatenate([ov.ravel(), ovp.ravel(), ljo.ravel(), lja, hist.ravel()]), dil


def _run(W, H, count):
    fr = _batch(W, H, count)
    pieces = np.array(PIECES[count], np.int32)
    planes = np.concatenate([np.concatenate([_pack(f[0]).ravel(), _pack(f[1]).ravel()]) for f in fr])
    occ2 = np.ascontiguousarray(np.stack([f[2] for f in fr])); dn = np.ascontiguousarray(np.stack([f[3] for f in fr]))
    sizes = [3 * c * c + c + 256 * c for c in pieces]; off = np.concatenate([[0], np.cumsum(sizes)])
    ob = np.full(off[-1], -7, np.int32); of = np.full(off[-1], -9, np.int32)
    check(lib().sind_debug_rag_batch(ptr(planes), ptr(pieces), ptr(occ2), ptr(dn), count, W, H, 0, ptr(ob), ptr(of)), "sind_debug_rag_batch")
    for i, f in enumerate(fr):
        b = ob[off[i]:off[i + 1]]; p = of[off[i]:off[i + 1]]
        assert b.tobytes() == p.tobytes(), (i, int((b != p).sum()))                # all five outputs: batched == per-frame kernels
        exp, dil = _expected(f, W, H)
        assert np.array_equal(b.astype(np.int64), exp), (i, np.flatnonzero(b != exp)[:8])
        Cn = int(pieces[i])
        if i == 0 and Cn >= 2:                                                     # two identical pieces: their overlap is the dilated area
            assert b[1] == int(dil[0].sum()) > 0
        if i == 1:                                                                 # no connection plane; occ2 all set: overlapPlane == overlap
            assert not b[2 * Cn * Cn:3 * Cn * Cn + Cn].any() and np.array_equal(b[:Cn * Cn], b[Cn * Cn:2 * Cn * Cn])
        if i == 2:                                                                 # occ2 all clear
            assert not b[Cn * Cn:2 * Cn * Cn].any()
        assert not b[3 * Cn * Cn + Cn:].reshape(Cn, 256)[:, 255].any()
    if count == 5:
        assert ob[off[0]:off[1]].tobytes() == ob[off[4]:off[5]].tobytes()          # the repeated frame: the same bytes twice


@pytest.mark.parametrize("count", [1, 3, 5])
@pytest.mark.parametrize("size", [(64, 8), (128, 12)])
def test_batched_stage_equals_per_frame_kernels_and_numpy(size, count):
    """64 x 8: one word per row, the 7 x 7 element crosses the top and bottom edges at every row; 128 x 12: two words per row, cross-word shifts and the tail mask.
    Piece counts [1], [2, 64, 1], [3, 65, 64, 1, 3]: the frame that counts in global memory sits inside a chunk whose other frames count in LDS"""
    _run(size[0], size[1], count)


def test_batched_stage_production_size():
    """640 x 480 once: many pixels per workgroup, ten words per row"""
    _run(640, 480, 5)


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


_cache = {}


def _two_steps(frames, on, chunk=None, planes=-1):
    """three streams on two pool workers (more streams than workers: non-split rounds), T = 2, two steps -> (outputs per step, (switch, batched, fallback))"""
    from sindslam_amd.pipeline import Pipeline
    S, T = 3, 2
    sb, sd = _streams(frames, S)
    pipe = Pipeline(S, T, 640, 480, *K, 1500, 1.2, 8, 15, 5, orb_gray_rgb_order=1, host_threads=2)
    assert pipe.rag_batch() == (True, 0, 0)                                        # on by default
    pipe.set_rag_batch(on)
    if chunk is not None:
        pipe.set_rag_batch_chunk(chunk, planes)
    for s in range(S):
        pipe.prime(s, sb[s, 1], sb[s, 0])
    steps = []
    for step in range(2):
        lo = 2 + step * T
        pipe.process(sb[:, lo:lo + T], sd[:, lo:lo + T]); steps.append(_outputs(pipe))
    st = pipe.rag_batch(); pipe.close()
    return steps, st


def _off(frames):
    if "off" not in _cache:
        _cache["off"] = _two_steps(frames, False)
    return _cache["off"]


def test_pipeline_batch_on_equals_off(frames):
    """every output of two steps is equal with the batched stage and with the per-frame stage; all 12 frames go through batches, none falls back"""
    off, st_off = _off(frames)
    on, st_on = _two_steps(frames, True)
    assert st_off == (False, 0, 0) and st_on == (True, 12, 0)
    for step in range(2):
        _assert_same(on[step], off[step], step)
    assert (on[1][1] > 0).any()


def test_pipeline_chunks_of_two(frames):
    """chunk size 2 with three frames per round: a full chunk and a partial last one in every round"""
    off, _ = _off(frames)
    on, st = _two_steps(frames, True, chunk=2)
    assert st == (True, 12, 0)
    for step in range(2):
        _assert_same(on[step], off[step], step)


def test_pipeline_slab_too_small_falls_back(frames):
    """a slab of 8 input planes per frame (24 for the round, four pieces each on average): frames that find it full take the per-frame stage and are counted"""
    off, _ = _off(frames)
    on, st = _two_steps(frames, True, chunk=32, planes=8)
    assert st[0] is True and st[2] > 0 and st[1] + st[2] == 12
    for step in range(2):
        _assert_same(on[step], off[step], step)


def test_ragged_step_batch_on_equals_off(frames):
    """a ragged step as rounds (no per-stream chains): streams with 2, 1, 0 and 2 active frames; outputs, state hashes and state blobs are equal"""
    from sindslam_amd.pipeline import Pipeline
    S, T = 4, 2
    sb, sd = _streams(frames, S)
    got = {}
    for on in (True, False):
        pipe = Pipeline(S, T, 640, 480, *K, 1500, 1.2, 8, 15, 5, orb_gray_rgb_order=1, host_threads=2)
        pipe.set_chain_max_streams(0); pipe.set_state_hashing(True); pipe.set_rag_batch(on)
        for s in range(S):
            pipe.prime(s, sb[s, 1], sb[s, 0])
        pipe.set_active_frames(np.array([2, 1, 0, 2], np.int32))
        pipe.process(sb[:, 2:2 + T], sd[:, 2:2 + T])
        assert pipe.rag_batch() == (on, 5 if on else 0, 0)
        got[on] = (_outputs(pipe), pipe.state_hashes(), [pipe.get_state(s) for s in range(S)]); pipe.close()
    _assert_same(got[True][0], got[False][0], "ragged")
    h = got[True][1]
    assert np.array_equal(h, got[False][1]) and (h[0] != 0).any(axis=1).all()
    for s in range(S):
        assert np.array_equal(got[True][2][s], got[False][2][s]), s
