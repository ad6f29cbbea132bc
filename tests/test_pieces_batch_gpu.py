"""GPU: the round's batched piece stage through its parity entry (sind_debug_pieces_batch): the real PieceBatch in chunks, depth planes at non-uniform device offsets
(the stage's depth table), the host step (seg_pieces_order), k_piece_commit_frames / k_piece_paint_frames into a RagBatch's device slab and launch_rag_frames on it --
against the host function packed from the host into a RagBatch (a round without the switch) and against the numpy reference of pieces_ref.py, bit for bit: records,
piece and connection planes as the kernels left them in the slab ([0, C) / [C, 2C), zeros of a missing connection area included), pieceOf, and the RAG result block.
Every crafted scene in one batch at 192 x 136; batches of 1, 3 and 5 in chunks of 3 (a full and a partial chunk); 64 x 64 and 128 x 72; a mixed chunk at 640 x 480 whose
first frame exceeds the chain capacity and is packed from the host; more than 254 pieces; "the highest rank wins" on pixels two pieces share."""
import ctypes as C

import numpy as np
import pytest

import pieces_ref as R
import pieces_scene as S
from sindslam_amd._lib import check, lib, ptr

pytestmark = pytest.mark.gpu

SCENES = S.piece_scenes()
REFS = {}
E_CAPACITY = -5


def ref_of(name):
    if name not in REFS:
        REFS[name] = R.frame_ref(SCENES[name])
    return REFS[name]


def rag_ints(c):
    return 3 * c * c + c + 256 * c


def stats_inputs(f, b):
    """occ2 and the 8-bit normalised depth of a frame for the region-adjacency statistics: any bytes do, the same on both sides"""
    occ2 = np.zeros((f.h, f.w), np.uint8); occ2[:, (5 + b) % 13::13] = 255; occ2[(3 + b) % 11::11, :] = 255
    dn = (f.depth.astype(np.uint32) * 255 // max(int(f.depth.max()), 1)).astype(np.uint8)
    return occ2, dn


def pieces_batch(frames, chunk, cap=64):
    """-> per side (gpu, host) a list of (C, (error code, fell back, committed on the device), recs, vals, planes, conn, piece_of, rag block) per frame"""
    n = len(frames); w, h, scale = frames[0].w, frames[0].h, frames[0].scale; wpr = w // 64
    k = max(len(f.planes) for f in frames)
    planes = np.zeros((n, k, h, wpr), np.uint64)
    for b, f in enumerate(frames):
        assert (f.w, f.h, f.scale) == (w, h, scale)
        for i, m in enumerate(f.planes):
            planes[b, i] = S.bits(m)
    occ = np.ascontiguousarray(np.stack([S.bits(f.occ1) for f in frames])); edge = np.ascontiguousarray(np.stack([S.bits(f.edge) for f in frames]))
    depth = np.ascontiguousarray(np.stack([f.depth for f in frames]).astype(np.uint16))
    st = [stats_inputs(f, b) for b, f in enumerate(frames)]
    occ2 = np.ascontiguousarray(np.stack([s[0] for s in st])); dn = np.ascontiguousarray(np.stack([s[1] for s in st]))
    rag_cap = rag_ints(cap)
    sides = []
    for _ in range(2):
        sides.append([np.full((n, 4), -7, np.int32), np.full((n, cap, 12), -7, np.int32), np.full((n, cap, 2), -7, np.float32), np.zeros((n, cap, h, wpr), np.uint64),
                      np.zeros((n, cap, h, wpr), np.uint64), np.full((n, h, w), 251, np.uint8), np.full((n, rag_cap), -7, np.int32)])
    check(lib().sind_debug_pieces_batch(ptr(planes), k, ptr(occ), ptr(edge), ptr(depth), ptr(occ2), ptr(dn), n, w, h, C.c_float(scale), 0, chunk, cap, rag_cap,
                                        *[ptr(a) for a in sides[0] + sides[1]]), "sind_debug_pieces_batch")
    out = []
    for info, recs, vals, pl, cn, po, rag in sides:
        out.append([(int(info[b, 0]), (int(info[b, 1]), int(info[b, 2]), int(info[b, 3])), recs[b, :max(0, min(info[b, 0], cap))], vals[b, :max(0, min(info[b, 0], cap))], pl[b], cn[b], po[b],
                     rag[b, :rag_ints(max(0, min(int(info[b, 0]), cap)))]) for b in range(n)])
    return out


def check_frames(names, frames, refs, chunk):
    gpu, host = pieces_batch(frames, chunk)
    for b, (name, f, ref) in enumerate(zip(names, frames, refs)):
        for tag, side in (("gpu", gpu), ("host", host)):
            Cn, status, recs, vals, pl, cn, po, rag = side[b]
            assert status == ((0, 0, 1 if Cn > 0 else 0) if tag == "gpu" else (0, 0, 0)), (name, tag, status)          # no frame of these falls back; every frame with pieces was committed on the device
            R.assert_equal_to_ref((name, tag), f, ref, Cn, recs, vals, pl, cn, po, S.unbits)
        for x, y in zip(gpu[b][2:], host[b][2:]):
            assert x.tobytes() == y.tobytes(), name
        if gpu[b][0] > 0:          # the result block is whole: its connection areas are those of the planes (zeros for a piece without one)
            Cn, rag = gpu[b][0], gpu[b][7]
            assert (rag != -7).all() and len(rag) == rag_ints(Cn)
            la = rag[3 * Cn * Cn:3 * Cn * Cn + Cn]
            by_rank = {int(r[11]): i for i, r in enumerate(gpu[b][2])}
            assert [int(v) for v in la] == [int(np.count_nonzero(S.unbits(gpu[b][5][by_rank[r]], f.w))) for r in range(Cn)], (name, "connection areas")
    return gpu, host


def test_every_scene_in_one_batch_equals_host_and_reference():
    names = sorted(k for k in SCENES if SCENES[k].scale == 5000.0)
    assert len(names) >= 14
    gpu, _ = check_frames(names, [SCENES[k] for k in names], [ref_of(k) for k in names], 32)
    assert any(not r[6] for g in gpu for r in g[2]) and any(r[6] for g in gpu for r in g[2])          # pieces with and without a connection area went through the commit


@pytest.mark.parametrize("names", [["crowded"], ["no_pieces", "crowded", "ordinary"], ["ordinary", "crowded", "score_tie", "hole_and_island", "no_pieces"]], ids=["n1", "n3", "n5"])
def test_batches_of_one_three_and_five_in_chunks_of_three(names):
    """n = 5: a full and a partial chunk, whose last frame has no pieces; n = 3: the chunk begins with one"""
    check_frames(names, [SCENES[k] for k in names], [ref_of(k) for k in names], 3)


def test_the_other_depth_scale():
    check_frames(["depth_limits_1000"], [SCENES["depth_limits_1000"]], [ref_of("depth_limits_1000")], 3)


def cropped(f, w, h):
    """the scene at w x h where everything it sets fits (None: it does not)"""
    if f.planes[:, h:, :].any() or f.planes[:, :, w:].any() or f.occ1[h:, :].any() or f.occ1[:, w:].any():
        return None
    g = S.Frame(w, h, k=len(f.planes), scale=f.scale)
    g.planes = f.planes[:, :h, :w].copy(); g.occ1 = f.occ1[:h, :w].copy(); g.edge = f.edge[:h, :w].copy(); g.depth = np.ascontiguousarray(f.depth[:h, :w])
    return g


@pytest.mark.parametrize("size", S.CONTOUR_SIZES[:2], ids=lambda s: "%dx%d" % s)
def test_small_sizes_on_the_scenes_that_fit(size):
    """64 x 64: one word per row; the crafted frames that fit, and whole planes of the contour scenes as clusters (a piece that touches all four borders among them)"""
    w, h = size
    names, frames = [], []
    for k in sorted(SCENES):
        g = cropped(SCENES[k], w, h) if SCENES[k].scale == 5000.0 else None
        if g is not None:
            names.append(k); frames.append(g)
    for k in ("full", "border_blobs", "hole_and_island", "word_seams"):
        g = S.Frame(w, h); g.planes[0] = S.contour_scenes(w, h)[k]; g.depth[:] = (np.arange(h)[:, None] * 50 + np.arange(w)[None, :] * 9 + 700).astype(np.uint16)
        names.append("contour_" + k); frames.append(g)
    assert len(frames) >= 6
    refs = [R.frame_ref(f) for f in frames]
    assert sum(len(r[0]) > 0 for r in refs) >= 3
    check_frames(names, frames, refs, 4)


def embedded(f, w, h):
    g = S.Frame(w, h, k=len(f.planes), scale=f.scale); g.edge[:] = False
    g.planes[:, :f.h, :f.w] = f.planes; g.occ1[:f.h, :f.w] = f.occ1; g.edge[:f.h, :f.w] = f.edge; g.depth[:f.h, :f.w] = f.depth
    return g


def test_a_mixed_chunk_at_640x480_one_frame_fallen_back_one_on_the_device():
    """the comb's one contour does not fit a plane's chain: the frame reports it, runs the host function and is packed from the host into the SAME run of RAG slots as the
    frame behind it, whose planes the commit kernels wrote on the device.  Both equal the host side, RAG block included"""
    frames = [S.chain_overflow(), embedded(SCENES["ordinary"], 640, 480)]
    gpu, host = pieces_batch(frames, 3, cap=16)
    assert gpu[0][1] == (0, 1, 0) and gpu[1][1] == (0, 0, 1) and host[0][1] == (0, 0, 0) and host[1][1] == (0, 0, 0)
    assert gpu[0][0] == 1 and gpu[1][0] >= 3
    for b in range(2):
        assert gpu[b][0] == host[b][0]
        for x, y in zip(gpu[b][2:], host[b][2:]):
            assert x.tobytes() == y.tobytes(), b
        assert (gpu[b][7] != -7).all() and len(gpu[b][7]) == rag_ints(gpu[b][0])


def test_more_than_254_pieces_are_the_same_count_and_error_on_both_sides():
    f = S.too_many_pieces()
    gpu, host = pieces_batch([f, embedded(SCENES["length_50_51"], 384, 288)], 3, cap=8)
    assert gpu[0][0] == host[0][0] > 254
    assert gpu[0][1] == (E_CAPACITY, 0, 0) and host[0][1] == (E_CAPACITY, 0, 0)
    assert b"pieces exceed the 8-bit label range of the reference" in lib().sind_last_error() and str(gpu[0][0]).encode() in lib().sind_last_error()
    assert (gpu[0][6] == 251).all() and (host[0][6] == 251).all()
    assert gpu[1][0] == host[1][0] == 1 and gpu[1][1] == (0, 0, 1)          # the frame behind it in the chunk is whole
    for x, y in zip(gpu[1][2:], host[1][2:]):
        assert x.tobytes() == y.tobytes()


def test_the_highest_rank_wins_the_pixels_two_pieces_share():
    """an occlusion edge cuts a cluster in two; grown back by the 9 x 9 element inside the cluster, both pieces cover the cut: pieceOf there is the higher rank"""
    f = SCENES["occ_cuts_a_cluster"]; pieces, rank, ref_po, _ = ref_of("occ_cuts_a_cluster")
    assert len(pieces) == 2
    both = pieces[0]["img"] & pieces[1]["img"]
    assert both.sum() > 100 and (ref_po[both] == 1).all() and (ref_po[pieces[int(np.argmin(rank))]["img"] & ~both] == 0).all()
    gpu, host = pieces_batch([f], 3)
    assert gpu[0][1] == (0, 0, 1)
    po = gpu[0][6]
    assert (po[both] == 1).all() and np.array_equal(po, ref_po) and np.array_equal(po, host[0][6])
    assert (po[~(pieces[0]["img"] | pieces[1]["img"])] == 3).all()          # C + 1 where no piece is


def test_bad_arguments_are_refused():
    a = np.zeros(64 * 8, np.uint64); o = np.zeros(4096, np.int32)
    f = lib().sind_debug_pieces_batch
    outs = [ptr(o)] * 14
    assert f(ptr(a), 1, ptr(a), ptr(a), ptr(a), ptr(a), ptr(a), 1, 60, 8, C.c_float(5000.0), 0, 3, 4, 64, *outs) == -1          # width not a multiple of 64
    assert f(ptr(a), 1, ptr(a), ptr(a), ptr(a), ptr(a), ptr(a), 65, 64, 8, C.c_float(5000.0), 0, 3, 4, 64, *outs) == -1
    assert f(ptr(a), 1, ptr(a), ptr(a), ptr(a), ptr(a), ptr(a), 1, 64, 8, C.c_float(5000.0), 0, 0, 4, 64, *outs) == -1 and b"sind_debug_pieces_batch" in lib().sind_last_error()
