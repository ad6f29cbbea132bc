"""CPU: the piece extraction of SegAndMerge as the host states it (csrc/host/pieces.hpp through sindh_seg_pieces of libsind_host.so, border following through
sindh_find_contours) against the plain numpy reference of pieces_ref.py and the oracle, bit for bit; every scene's rule asserted from the reference's own record; every
scene but the overflow scenes inside the documented capacities of the device stage; a sanitizer build of the twin as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pieces_ref as R
import pieces_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host():
    so = os.path.join(ROOT, "sindslam_amd", "libsind_host.so")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sindslam_amd", "csrc"), "../libsind_host.so"])
    return C.CDLL(so)


H = host()
P = lambda a: a.ctypes.data_as(C.c_void_p)
CAPS = np.zeros(6, np.int32); H.sindh_piece_capacities(P(CAPS))          # the device stage's capacities as the library states them (pieces_dev.hpp)
CAP1, CAP2, SLOTS, KMAX = (int(CAPS[0]), int(CAPS[1])), (int(CAPS[2]), int(CAPS[3])), int(CAPS[4]), int(CAPS[5])
SCENES = S.piece_scenes()
REFS = {}


def ref_of(name):
    if name not in REFS:
        REFS[name] = R.frame_ref(SCENES[name])
    return REFS[name]


def host_seg_pieces(f, cap=64):
    k = len(f.planes); wpr = (f.w + 63) // 64
    planes = np.ascontiguousarray(np.stack([S.bits(m) for m in f.planes]))
    recs = np.full((cap, 12), -7, np.int32); vals = np.full((cap, 2), -7, np.float32)
    pl = np.zeros((cap, f.h, wpr), np.uint64); cn = np.zeros((cap, f.h, wpr), np.uint64); po = np.full((f.h, f.w), 251, np.uint8)
    n = H.sindh_seg_pieces(P(planes), k, P(S.bits(f.occ1)), P(S.bits(f.edge)), P(np.ascontiguousarray(f.depth)), f.w, f.h, C.c_float(f.scale), cap, P(recs), P(vals), P(pl), P(cn), P(po))
    return n, recs[:min(n, cap)], vals[:min(n, cap)], pl, cn, po


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_equals_the_reference(name):
    f = SCENES[name]
    n, recs, vals, pl, cn, po = host_seg_pieces(f)
    R.assert_equal_to_ref(name, f, ref_of(name), n, recs, vals, pl, cn, po, S.unbits)


def test_every_scene_shows_its_rule():
    assert S.CONTOUR_CAPS == CAP1 and SLOTS >= 255 and KMAX >= max(len(f.planes) for f in SCENES.values())
    lens = lambda name: sorted(c[1] for c in ref_of(name)[3])
    assert lens("length_50_51") == [50, 51] and [p["clen"] for p in ref_of("length_50_51")[0]] == [51]
    c = ref_of("area_160_161_162")[3]
    assert sorted(q[2] for q in c) == [160, 161, 162] and all(q[1] > 50 for q in c) and sorted(p["sum2"] for p in ref_of("area_160_161_162")[0]) == [161, 162]
    c = ref_of("thin_and_square")[3]
    assert len(c) == 2 and not ref_of("thin_and_square")[0]
    assert any(q[1] > 50 and q[2] <= 160 for q in c) and any(q[1] <= 50 and q[2] > 160 for q in c)
    pieces = ref_of("hole_and_island")[0]; f = SCENES["hole_and_island"]
    ring = [p for p in pieces if p["cluster"] == 0]
    assert len(ring) == 1 and ring[0]["img"][45, 50] and not ring[0]["img"][37, 40]          # the island joined; the hole, which the fill closed, is open again
    assert R.fill_even_odd(f.occ1.shape, [O.find_contours(O.morph(R.u8(f.planes[0]), 4, "open"), True)[0]])[37, 40] and not f.planes[0][37, 40]
    assert [p["cluster"] for p in ref_of("occ_cuts_a_cluster")[0]] == [0, 0]
    assert sorted(p["band_count"] for p in ref_of("band_20_21")[0]) == [20, 21] and [bool(p["contours2"]) for p in sorted(ref_of("band_20_21")[0], key=lambda p: p["band_count"])] == [False, True]
    p2 = ref_of("second_level_29_30")[0]
    assert sorted(tuple(p["contours2"]) for p in p2) == [(29,), (30,)] and sorted(p["has_conn"] for p in p2) == [False, True]
    assert [float(p["cz"]) for p in ref_of("no_valid_depth")[0]] == [0.0]
    # Several kept second-level contours share one plane.  They are external borders of ONE plane: a component inside a hole of another is not reported, so their fills
    # never overlap and even-odd over all of them together equals the union of the single fills -- asserted here on every piece of every scene that keeps two or more
    seen = 0
    for name in SCENES:
        f = SCENES[name]; occ_dil = O.morph(R.u8(f.occ1), 10, "dilate") > 0
        for p in ref_of(name)[0]:
            if sum(L >= 30 for L in p["contours2"]) < 2:
                continue
            seen += 1
            c = [q for q in O.find_contours(O.morph(R.u8(f.planes[p["cluster"]] & ~f.occ1), 4, "open"), True) if (int(q[0][0]), int(q[0][1])) == p["start"]][0]
            kept = [q for q in O.find_contours(R.u8(R.band(f.occ1.shape, c) & ~occ_dil & f.edge), True) if len(q) >= 30]
            fills = [R.fill_even_odd(f.occ1.shape, [q]) for q in kept]
            assert np.sum(fills, axis=0).max() == 1 and np.array_equal(np.any(fills, axis=0), p["conn"]), name
    assert seen >= 1 and len(ref_of("two_kept_contours")[0][0]["contours2"]) == 3
    for scale in (5000, 1000):
        f = SCENES["depth_limits_%d" % scale]; p = ref_of("depth_limits_%d" % scale)[0][0]; zi = S.z_invalid_from(float(scale))
        t = R.depth_terms(f.depth, f.scale)
        assert t[40, 26] == 0 and t[41, 26] == 0 and (t[42, 26] > 0) and t[43, 26] == 0 and f.depth[42, 26] == zi - 1 and p["img"][40:44, 25:30].all()
    p = ref_of("sequential_sum")[0][0]
    assert R.sequential_sum(p["terms"]) != R.pairwise_sum(p["terms"])
    a, b = ref_of("score_tie")[0]
    assert a["score"] == b["score"] and a["area"] == b["area"] and a["cz"] == b["cz"]
    assert ref_of("no_pieces")[0] == [] and ref_of("no_pieces")[3] == []
    assert len(ref_of("crowded")[0]) > 16 and R.rank_is_defined(ref_of("crowded")[0])          # beyond the insertion-sort range of std::sort, all scores distinct


def test_more_than_254_pieces_are_counted_and_not_ranked():
    f = S.too_many_pieces()
    n, recs, vals, pl, cn, po = host_seg_pieces(f, cap=4)
    ref = R.frame_ref(f)
    assert n == len(ref[0]) > 254 and ref[1] is None and (po == 251).all() and (recs[:, 11] == -1).all()


@pytest.mark.parametrize("size", S.CONTOUR_SIZES, ids=lambda s: "%dx%d" % s)
def test_host_contours_equal_the_oracle(size):
    w, h = size
    for name, m in S.contour_scenes(w, h).items():
        img = R.u8(m); pts = np.zeros((w * h * 4, 2), np.int32); lens = np.zeros(w * h, np.int32)
        n = H.sindh_find_contours(P(img), w, h, 1, P(pts), len(pts), P(lens), len(lens))
        ref = O.find_contours(img, True)
        assert n == len(ref) and list(lens[:n]) == [len(c) for c in ref], name
        assert np.array_equal(pts[:sum(lens[:n])], np.concatenate(ref) if ref else np.zeros((0, 2), np.int32)), name
        assert n <= CAP1[0] and sum(lens[:n]) <= CAP1[1], name          # inside the device capacities: the overflow tests pass smaller ones


def test_every_scene_stays_inside_the_device_capacities():
    """what keeps a silent fallback from hiding a failure: no scene but the overflow scenes can exceed a capacity of the device stage"""
    for name, f in list(SCENES.items()) + [("synthetic", S.synthetic_frame())]:
        ref = ref_of(name) if name in SCENES else R.frame_ref(f)
        per_plane = {}
        for i, L, _ in ref[3]:
            c = per_plane.setdefault(i, [0, 0]); c[0] += 1; c[1] += L
        assert all(c[0] <= CAP1[0] and c[1] <= CAP1[1] for c in per_plane.values()), name
        assert all(len(p["contours2"]) <= CAP2[0] and sum(p["contours2"]) <= CAP2[1] for p in ref[0]), name
        assert len(ref[0]) <= 254, name
    over = R.frame_ref(S.chain_overflow())
    assert sum(L for _, L, _ in over[3]) > CAP1[1]


def test_a_sanitizer_build_of_the_host_twin_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_find_contours / sindh_seg_pieces with -fsanitize=address,undefined, run as a program of its own on three scenes; it prints the piece count
    and a checksum of every output, which must be what the library loaded here gives"""
    exe = str(tmp_path / "pieces_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sindslam_amd", "csrc"), "sanitize-pieces", "OUT=" + exe], check=True, capture_output=True, text=True)
    for name in ("ordinary", "second_level_29_30", "crowded"):
        f = SCENES[name]; k = len(f.planes); path = tmp_path / (name + ".bin")
        with open(path, "wb") as fh:
            fh.write(np.array([f.w, f.h, k, int(f.scale)], np.int32).tobytes())
            for m in f.planes:
                fh.write(S.bits(m).tobytes())
            fh.write(S.bits(f.occ1).tobytes()); fh.write(S.bits(f.edge).tobytes()); fh.write(np.ascontiguousarray(f.depth).tobytes())
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (name, r.returncode, r.stderr[-2000:])
        n, recs, vals, pl, cn, po = host_seg_pieces(f)
        sums = [int(a[:n].view(np.uint8).astype(np.uint64).sum()) if a is not po else int(a.astype(np.uint64).sum()) for a in (recs, vals, pl, cn, po)]
        ncont = sum(len(O.find_contours(R.u8(m), True)) for m in f.planes)
        assert [int(v) for v in r.stdout.split()] == [n] + sums + [ncont], (name, r.stdout)
