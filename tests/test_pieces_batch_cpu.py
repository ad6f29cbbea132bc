"""CPU: the host step between the two device steps of the batched piece stage -- records of a frame in discovery order -> the pieces' rank order and the order table
the commit kernels read (seg_pieces_order of csrc/host/pieces.hpp through sindh_seg_pieces_order of libsind_host.so) -- against the ranking of pieces_ref.py and
against the host function's own ranking on the same discovery sequence (sindh_seg_pieces), on every scene of pieces_scene.piece_scenes(); frames of 0, 254 and 255
pieces; a sanitizer build as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pieces_ref as R
import pieces_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host():
    so = os.path.join(ROOT, "sindslam_amd", "libsind_host.so")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sindslam_amd", "csrc"), "../libsind_host.so"])
    return C.CDLL(so)


H = host()
P = lambda a: a.ctypes.data_as(C.c_void_p)
SCENES = S.piece_scenes()
REFS = {}


def ref_of(name):
    if name not in REFS:
        REFS[name] = R.frame_ref(SCENES[name])
    return REFS[name]


def records(pieces):
    """the reference's pieces in discovery order as the device stage's records: [C][16] int32 (cz as float bits)"""
    recs = np.zeros((len(pieces), 16), np.int32)
    for i, p in enumerate(pieces):
        recs[i, :9] = [p["cluster"], i, p["start"][0], p["start"][1], p["clen"], *p["box"]]
        recs[i, 9:11] = np.array([p["sum2"] & 0xffffffff, p["sum2"] >> 32], np.uint32).view(np.int32)
        recs[i, 11:14] = [int(p["area"]), p["band_count"], int(p["has_conn"])]
        recs[i, 14] = np.array([p["cz"]], np.float32).view(np.int32)[0]
    return recs


def order_of(recs):
    order = np.full(255, -7, np.int32); conn = np.full(255, -7, np.int32); score = np.full(255, -7, np.float32)
    n = H.sindh_seg_pieces_order(P(recs) if len(recs) else None, len(recs), P(order), P(conn), P(score))
    return n, order, conn, score


def host_rank(f, cap=64):
    """rank of every piece (discovery order) as the host function's path sorts them: sindh_seg_pieces on the scene"""
    k = len(f.planes); wpr = (f.w + 63) // 64
    planes = np.ascontiguousarray(np.stack([S.bits(m) for m in f.planes]))
    recs = np.full((cap, 12), -7, np.int32); vals = np.full((cap, 2), -7, np.float32)
    pl = np.zeros((cap, f.h, wpr), np.uint64); cn = np.zeros((cap, f.h, wpr), np.uint64); po = np.full((f.h, f.w), 251, np.uint8)
    n = H.sindh_seg_pieces(P(planes), k, P(S.bits(f.occ1)), P(S.bits(f.edge)), P(np.ascontiguousarray(f.depth)), f.w, f.h, C.c_float(f.scale), cap, P(recs), P(vals), P(pl), P(cn), P(po))
    assert 0 <= n <= cap
    return [int(v) for v in recs[:n, 11]]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_order_table_equals_the_reference_and_the_host_function(name):
    pieces, rank, _, _ = ref_of(name)
    n, order, conn, score = order_of(records(pieces))
    assert n == len(pieces)
    assert (order[n:] == -7).all() and (conn[n:] == -7).all() and (score[n:] == -7).all()          # nothing behind the frame's pieces is written
    if n == 0:
        assert name in ("no_pieces", "thin_and_square") and rank is None          # the two scenes without a piece: nothing is ranked
        return
    assert sorted(order[:n]) == list(range(n))
    hr = host_rank(SCENES[name])                                        # the host function's own order on the same discovery sequence: ties included
    assert [hr[order[r]] for r in range(n)] == list(range(n)), (name, order[:n], hr)
    assert [int(conn[r]) for r in range(n)] == [int(pieces[order[r]]["has_conn"]) for r in range(n)]
    assert score[:n].tobytes() == np.array([pieces[order[r]]["score"] for r in range(n)], np.float32).tobytes()
    assert all(score[r] >= score[r + 1] for r in range(n - 1))
    if R.rank_is_defined(pieces):
        assert [int(rank[order[r]]) for r in range(n)] == list(range(n)), (name, "reference rank")


def test_equal_scores_keep_the_host_functions_order():
    pieces = ref_of("score_tie")[0]
    assert len(pieces) == 2 and pieces[0]["score"] == pieces[1]["score"]
    n, order, _, score = order_of(records(pieces))
    assert n == 2 and score[0] == score[1] and [host_rank(SCENES["score_tie"])[order[r]] for r in range(2)] == [0, 1]


def synthetic_records(n):
    r = np.random.RandomState(n); recs = np.zeros((n, 16), np.int32)
    recs[:, 0] = np.sort(r.randint(0, 12, n)); recs[:, 1] = np.arange(n); recs[:, 4] = 60; recs[:, 11] = r.randint(100, 30000, n); recs[:, 13] = r.randint(0, 2, n)
    recs[:, 14] = r.uniform(0.2, 8.0, n).astype(np.float32).view(np.int32)
    return recs


def test_frames_of_0_254_and_255_pieces():
    n, order, conn, score = order_of(np.zeros((0, 16), np.int32))
    assert n == 0 and (order == -7).all() and (conn == -7).all()
    recs = synthetic_records(254)
    n, order, conn, score = order_of(recs)
    assert n == 254 and sorted(order[:254]) == list(range(254)) and order[254] == -7
    want = (recs[:, 11].astype(np.float32) * np.float32(0.0003)).astype(np.float32) - recs[:, 14].view(np.float32)
    assert score[:254].tobytes() == want.astype(np.float32)[order[:254]].tobytes() and all(score[r] >= score[r + 1] for r in range(253))
    assert [int(v) for v in conn[:254]] == [int(v) for v in recs[order[:254], 13]]
    n, order, conn, score = order_of(synthetic_records(255))          # beyond the 8-bit label range: refused, nothing written
    assert n == -1 and (order == -7).all() and (conn == -7).all() and (score == -7).all()


def test_a_sanitizer_build_of_the_host_step_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_seg_pieces_order with -fsanitize=address,undefined, run as a program of its own on the scenes' records and on 0, 254 and 255 synthetic ones;
    its tables have exactly 255 entries.  What it prints must be what the library loaded here gives"""
    exe = str(tmp_path / "pieces_batch_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sindslam_amd", "csrc"), "sanitize-pieces-batch", "OUT=" + exe], check=True, capture_output=True, text=True)
    frames = [records(ref_of(k)[0]) for k in ("ordinary", "crowded", "score_tie", "no_pieces")] + [synthetic_records(254), synthetic_records(255)]
    path = tmp_path / "frames.bin"
    with open(path, "wb") as fh:
        for recs in frames:
            fh.write(np.array([len(recs)], np.int32).tobytes()); fh.write(np.ascontiguousarray(recs).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(frames)
    for recs, line in zip(frames, lines):
        n, order, conn, score = order_of(recs)
        want = [n]
        for q in range(max(n, 0)):
            want += [int(order[q]), int(conn[q]), int(score[q:q + 1].view(np.uint32)[0])]
        assert [int(v) for v in line.split()] == want
