"""GPU: the device side of SegAndMerge's piece extraction against the host function and the oracle, bit for bit.  Border following (k_piece_contours through
sind_debug_contours): every scene of pieces_scene.contour_scenes at 64 x 64 (one word per row), 128 x 72 and 192 x 136 in ONE launch per size, a 640 x 480 plane (the cells
fill 77 KB of LDS), a 1280 x 720 plane (the cells lie in global memory), and both capacities exceeded.  The whole stage through sind_debug_seg_pieces: several frames run in one
batched PieceStage; ONE frame runs through a tail of its own with the switch on (pinned staging, capacity-1 stage on the tail's stream, fallback, ranking, k_piece_commit:
planes and pieceOf come back from the device in the RAG stage's layout).  Every frame of pieces_scene.piece_scenes in one batch and each through the tail, batches of 3 and 5,
more than 254 pieces at 384 x 288 on both paths (the tail's error text included), a 640 x 480 frame of the synthetic stream, and a frame beyond the chain capacity, which
falls back in the tail with equal results and the counters (0, 1).  device == host == numpy reference, bit for bit.  The rules the scenes are made for are asserted in
test_pieces_cpu.py from the reference alone."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pieces_ref as R
import pieces_scene as S
from sindslam_amd._lib import check, lib, ptr

pytestmark = pytest.mark.gpu


def debug_contours(planes, w, cap_contours=S.CONTOUR_CAPS[0], cap_points=S.CONTOUR_CAPS[1]):
    """planes: list of bool [h][w] -> per side (gpu, host): counts [n][3], hdr [n][cap_contours][10], pts [n][cap_points][2]"""
    n = len(planes); h = planes[0].shape[0]
    words = np.ascontiguousarray(np.stack([S.bits(m) for m in planes]))
    out = []
    for _ in range(2):
        out += [np.full((n, 3), -7, np.int32), np.full((n, cap_contours, 10), -7, np.int32), np.full((n, cap_points, 2), -7, np.int32)]
    check(lib().sind_debug_contours(ptr(words), n, w, h, 0, cap_contours, cap_points, *[ptr(a) for a in out]), "sind_debug_contours")
    return out[:3], out[3:]


def contours_of(counts, hdr, pts, i):
    return [pts[i, hdr[i, k, 3]:hdr[i, k, 3] + hdr[i, k, 2]] for k in range(counts[i, 0])]


def check_plane(name, m, gpu, host, i):
    ref = O.find_contours(m.astype(np.uint8) * 255, True)
    for side, (counts, hdr, pts) in (("gpu", gpu), ("host", host)):
        assert counts[i, 2] == 0, (name, side, counts[i])
        assert counts[i, 0] == len(ref) and counts[i, 1] == sum(len(c) for c in ref), (name, side, counts[i], len(ref))
        got = contours_of(counts, hdr, pts, i)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(a, b), (name, side, k)
            c = np.asarray(b, np.int64); p = np.roll(c, 1, axis=0); s2 = int(abs(np.sum(p[:, 0] * c[:, 1] - p[:, 1] * c[:, 0])))
            want = [c[0, 0], c[0, 1], len(c), sum(len(q) for q in ref[:k]), c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max(), s2 & 0xffffffff, s2 >> 32]
            assert [int(v) & 0xffffffff for v in hdr[i, k]] == [int(v) & 0xffffffff for v in want], (name, side, k, hdr[i, k], want)
    assert np.array_equal(gpu[0][i], host[0][i]) and np.array_equal(gpu[1][i], host[1][i]) and np.array_equal(gpu[2][i], host[2][i]), name


@pytest.mark.parametrize("size", S.CONTOUR_SIZES, ids=lambda s: "%dx%d" % s)
def test_contours_equal_host_and_oracle_on_every_scene(size):
    w, h = size
    scenes = S.contour_scenes(w, h)
    names = sorted(scenes)
    gpu, host = debug_contours([scenes[k] for k in names], w)
    for i, k in enumerate(names):
        check_plane(k, scenes[k], gpu, host, i)
    many = names.index("many_components"); comb = names.index("comb")
    assert gpu[0][many, 0] > 300, gpu[0][many]
    assert gpu[0][comb, 1] > 2000, gpu[0][comb]


def blobs(w, h, seed):
    """random rectangles and holes: a busy plane at a production size"""
    r = np.random.RandomState(seed); m = np.zeros((h, w), bool)
    for _ in range(60):
        x, y, a, b = r.randint(0, w - 8), r.randint(0, h - 8), r.randint(2, w // 5), r.randint(2, h // 5); m[y:y + b, x:x + a] = True
    for _ in range(40):
        x, y, a, b = r.randint(0, w - 8), r.randint(0, h - 8), r.randint(1, w // 12), r.randint(1, h // 12); m[y:y + b, x:x + a] = False
    m[r.randint(0, h, 300), r.randint(0, w, 300)] = True
    return m


@pytest.mark.parametrize("size", [(640, 480), (1280, 720)], ids=lambda s: "%dx%d" % s)
def test_contours_at_production_sizes(size):
    """640 x 480: the cells are in LDS; 1280 x 720: in the global scratch plane.  Three planes in one launch: busy, empty, full"""
    w, h = size
    planes = [blobs(w, h, 5), np.zeros((h, w), bool), np.ones((h, w), bool)]
    gpu, host = debug_contours(planes, w)
    for i, m in enumerate(planes):
        check_plane("plane %d" % i, m, gpu, host, i)
    assert gpu[0][0, 0] > 50


@pytest.mark.parametrize("name", sorted(S.OVERFLOW))
def test_a_plane_beyond_a_capacity_stops_with_its_status(name):
    """the device stops at the capacity and says which; what it wrote up to there is the beginning of the host's answer.  The other plane of the launch is not disturbed"""
    w, h = 128, 72
    cap_c, cap_p, status = S.OVERFLOW[name]
    scenes = S.contour_scenes(w, h)
    gpu, host = debug_contours([scenes[name], scenes["hole_and_island"]], w, cap_c, cap_p)
    assert gpu[0][0, 2] == status and host[0][0, 2] == status, (gpu[0][0], host[0][0])
    assert host[0][0, 0] > cap_c or host[0][0, 1] > cap_p
    nc, npts = gpu[0][0, 0], gpu[0][0, 1]
    assert 0 <= nc <= cap_c and 0 <= npts <= cap_p
    assert np.array_equal(gpu[1][0, :nc], host[1][0, :nc]) and np.array_equal(gpu[2][0, :npts], host[2][0, :npts])
    check_plane("second plane", scenes["hole_and_island"], gpu, host, 1)


def test_bad_arguments_are_refused():
    a = np.zeros(64, np.uint64); o = np.zeros(64, np.int32)
    f = lib().sind_debug_contours
    assert f(None, 1, 64, 8, 0, 4, 4, ptr(o), ptr(o), ptr(o), ptr(o), ptr(o), ptr(o)) == -1
    assert f(ptr(a), 0, 64, 8, 0, 4, 4, ptr(o), ptr(o), ptr(o), ptr(o), ptr(o), ptr(o)) == -1
    assert f(ptr(a), 1, 64, 8, 0, 0, 4, ptr(o), ptr(o), ptr(o), ptr(o), ptr(o), ptr(o)) == -1 and b"sind_debug_contours" in lib().sind_last_error()


# ---------------------------------------------------------------------------------------------------------------- the whole stage
SCENES = S.piece_scenes()
REFS = {}


def ref_of(name):
    if name not in REFS:
        REFS[name] = R.frame_ref(SCENES[name])
    return REFS[name]


def debug_seg_pieces(frames, cap=64):
    """frames of one size and depth scale (fewer planes are padded with empty ones) -> per side (gpu, host) a list of (C, (status, frames on the device, frames fallen back), recs, vals, planes, conn, piece_of)
    per frame.  ONE frame goes through a tail of its own with the switch on (capacity-1 stage on its stream, fallback, ranking, k_piece_commit); more through one batched object"""
    n = len(frames); w, h, scale = frames[0].w, frames[0].h, frames[0].scale; wpr = (w + 63) // 64
    k = max(len(f.planes) for f in frames)
    planes = np.zeros((n, k, h, wpr), np.uint64)
    for b, f in enumerate(frames):
        assert (f.w, f.h, f.scale) == (w, h, scale)
        for i, m in enumerate(f.planes):
            planes[b, i] = S.bits(m)
    occ = np.ascontiguousarray(np.stack([S.bits(f.occ1) for f in frames])); edge = np.ascontiguousarray(np.stack([S.bits(f.edge) for f in frames]))
    depth = np.ascontiguousarray(np.stack([f.depth for f in frames]).astype(np.uint16))
    sides = []
    for _ in range(2):
        sides.append([np.full((n, 4), -7, np.int32), np.full((n, cap, 12), -7, np.int32), np.full((n, cap, 2), -7, np.float32), np.zeros((n, cap, h, wpr), np.uint64),
                      np.zeros((n, cap, h, wpr), np.uint64), np.full((n, h, w), 251, np.uint8)])
    check(lib().sind_debug_seg_pieces(ptr(planes), k, ptr(occ), ptr(edge), ptr(depth), n, w, h, C.c_float(scale), 0, cap, *[ptr(a) for a in sides[0] + sides[1]]), "sind_debug_seg_pieces")
    out = []
    for info, recs, vals, pl, cn, po in sides:
        out.append([(int(info[b, 0]), (int(info[b, 1]), int(info[b, 2]), int(info[b, 3])), recs[b, :max(0, min(info[b, 0], cap))], vals[b, :max(0, min(info[b, 0], cap))], pl[b], cn[b], po[b]) for b in range(n)])
    return out


def check_frames(names, frames, refs):
    gpu, host = debug_seg_pieces(frames)
    for b, (name, f, ref) in enumerate(zip(names, frames, refs)):
        for tag, side in (("gpu", gpu), ("host", host)):
            Cn, status, recs, vals, pl, cn, po = side[b]
            want = ((0, 1, 0) if ref[0] else (0, 1, 0)) if tag == "gpu" and len(frames) == 1 else (0, 0, 0)
            assert status == want, (name, tag, status)          # no frame of these falls back; through the tail, the frame is counted as cut on the device
            R.assert_equal_to_ref((name, tag), f, ref, Cn, recs, vals, pl, cn, po, S.unbits)
        for x, y in zip(gpu[b][2:], host[b][2:]):
            assert x.tobytes() == y.tobytes(), name


def test_every_scene_in_one_batch_equals_host_and_reference():
    names = sorted(k for k in SCENES if SCENES[k].scale == 5000.0)
    check_frames(names, [SCENES[k] for k in names], [ref_of(k) for k in names])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_scene_through_the_tail(name):
    """n = 1: the tail's own path with the switch on -- pinned staging, the capacity-1 stage on the tail's stream, records, ranking, k_piece_commit: the planes come back from
    the RAG stage's layout in rank order and pieceOf from the device -- on every crafted rule"""
    check_frames([name], [SCENES[name]], [ref_of(name)])


@pytest.mark.parametrize("names", [["no_pieces", "crowded", "ordinary"], ["ordinary", "no_pieces", "score_tie", "crowded", "hole_and_island"]], ids=["n3", "n5"])
def test_batches_of_three_and_five(names):
    check_frames(names, [SCENES[k] for k in names], [ref_of(k) for k in names])


@pytest.mark.parametrize("n", [1, 2], ids=["tail", "batched"])
def test_more_than_254_pieces_are_the_same_count_on_both_sides(n):
    f = S.too_many_pieces()
    gpu, host = debug_seg_pieces([f] * n, cap=8)
    assert gpu[0][0] == host[0][0] == len(R.frame_ref(f)[0]) > 254
    assert (host[0][2][:, 11] == -1).all() and (gpu[0][6] == 251).all() and (host[0][6] == 251).all()
    if n > 1:
        assert (gpu[0][2][:, 11] == -1).all()
    else:                 # the tail refused the frame with the host path's words (and hands out no records)
        assert b"pieces exceed the 8-bit label range of the reference" in lib().sind_last_error() and gpu[0][1] == (0, 1, 0)


def test_a_frame_of_the_synthetic_stream_at_640x480():
    f = S.synthetic_frame()
    ref = R.frame_ref(f)
    assert len(ref[0]) >= 3
    check_frames(["synthetic"], [f], [ref])
    check_frames(["synthetic", "synthetic"], [f, f], [ref, ref])


def test_a_frame_beyond_the_chain_capacity_falls_back_with_equal_results():
    """the comb's one contour does not fit a plane's chain.  Through the tail (n = 1) the frame falls back to the host function: the results equal the host's and the
    reference's and the counters read (0 on the device, 1 fallen back).  Batched, the device stage reports the status and the host side is whole"""
    f = S.chain_overflow(); ref = R.frame_ref(f)
    assert len(ref[0]) == 1
    gpu, host = debug_seg_pieces([f], cap=8)
    assert gpu[0][1] == (1, 0, 1) and host[0][1] == (0, 0, 0)
    for tag, side in (("tail", gpu), ("host", host)):
        Cn, _, recs, vals, pl, cn, po = side[0]
        R.assert_equal_to_ref(("overflow", tag), f, ref, Cn, recs, vals, pl, cn, po, S.unbits)
    for x, y in zip(gpu[0][2:], host[0][2:]):
        assert x.tobytes() == y.tobytes()
    gpu2, host2 = debug_seg_pieces([f, SCENES["ordinary"].__class__(640, 480)], cap=8)
    assert gpu2[0][1][0] != 0 and gpu2[1][1][0] == 0 and host2[0][0] == 1
