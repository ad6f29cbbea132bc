"""Plain numpy restatement of the piece extraction of SegAndMergeV2 (reference DynaDetect.cc:664-729) and of the ranking behind it (:733-752).

The two primitives the oracle exposes are taken from it (oracle_lib.find_contours, oracle_lib.morph); the FILLED drawing (boundary plus even-odd interior per
scanline), the thickness-2 drawing (every contour pixel and its four neighbours) and the sequential float32 depth sum are written out here.  Nothing is shared with
csrc/host/contours.hpp, csrc/host/pieces.hpp or the kernels."""
import numpy as np

import oracle_lib as O

F = np.float32


def fill_even_odd(shape, contours):
    """cv::drawContours(FILLED) of closed unit-step chains sharing one edge table: an edge that changes row crosses the scanline of its upper end at that end's column;
    the sorted crossings of a row are filled pairwise, ends included; every chain pixel is set"""
    h, w = shape; out = np.zeros(shape, bool); rows = {}
    for c in contours:
        c = np.asarray(c); nxt = np.roll(c, -1, axis=0)
        out[c[:, 1], c[:, 0]] = True
        for (x0, y0), (x1, y1) in zip(c, nxt):
            if y0 != y1:
                rows.setdefault(min(y0, y1), []).append(x0 if y0 < y1 else x1)
    for y, xs in rows.items():
        xs = sorted(xs)
        for a, b in zip(xs[0::2], xs[1::2]):
            out[y, a:b + 1] = True
    return out


def band(shape, contour):
    """cv::drawContours(thickness 2) of a unit-step chain: the five-pixel cross around every point, clipped"""
    h, w = shape; out = np.zeros(shape, bool); c = np.asarray(contour)
    for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
        x = c[:, 0] + dx; y = c[:, 1] + dy; ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        out[y[ok], x[ok]] = True
    return out


def area2(contour):
    """twice cv::contourArea: |sum of x[i-1] y[i] - y[i-1] x[i]| over the closed chain (integers)"""
    c = np.asarray(contour, np.int64); p = np.roll(c, 1, axis=0)
    return int(abs(np.sum(p[:, 0] * c[:, 1] - p[:, 1] * c[:, 0])))


def depth_terms(depth, depth_scale):
    """what a pixel adds to a piece's z sum: (float)d * (1 / depthScale) * 1.5, 0 for a raw depth of 0 or one that is 6 m or more"""
    d = depth.astype(F); z = d / F(depth_scale)
    t = (d * (F(1.0) / F(depth_scale))) * F(1.5)
    return np.where((depth == 0) | (z >= F(6)), F(0), t).astype(F)


def sequential_sum(v):
    return F(np.add.accumulate(np.asarray(v, F), dtype=F)[-1]) if len(v) else F(0)


def pairwise_sum(v):
    v = list(np.asarray(v, F))
    while len(v) > 1:
        v = [F(v[i] + v[i + 1]) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else F(0)


def u8(m):
    return np.ascontiguousarray(m.astype(np.uint8) * 255)


def seg_pieces(planes, occ1, label_edge, depth, depth_scale):
    """planes [K][H][W] bool (all are cut), occ1 / label_edge [H][W] bool (the latter already dilated), depth [H][W] u16 -> (pieces in discovery order, rank, piece_of, candidates = (plane, length, twice the area) of every contour).
    A piece: cluster, start, clen, sum2, box, area, cz, has_conn, img, conn, band_count, contours2 (lengths of the second-level contours), terms (its z terms in order)"""
    shape = occ1.shape
    occ_dil = O.morph(u8(occ1), 10, "dilate") > 0
    terms = depth_terms(depth, depth_scale)
    pieces = []; cands = []
    for i, orig in enumerate(planes):
        each = O.morph(u8(orig & ~occ1), 4, "open")
        for c in O.find_contours(each, True):
            s2 = area2(c); cands.append((i, len(c), s2))
            if not (len(c) > 50 and s2 * 0.5 > 80):
                continue
            img = (O.morph(u8(fill_even_odd(shape, [c])), 9, "dilate") > 0) & orig
            t1 = band(shape, c) & ~occ_dil & label_edge
            p = dict(cluster=i, start=(int(c[0][0]), int(c[0][1])), clen=len(c), sum2=s2, box=(int(c[:, 0].min()), int(c[:, 1].min()), int(c[:, 0].max()), int(c[:, 1].max())),
                     area=F(np.count_nonzero(img)), img=img, has_conn=False, conn=np.zeros(shape, bool), band_count=int(np.count_nonzero(t1)), contours2=[])
            if p["band_count"] > 20:
                c2 = O.find_contours(u8(t1), True)
                p["contours2"] = [len(q) for q in c2]
                kept = [q for q in c2 if len(q) >= 30]
                if kept:
                    p["has_conn"] = True; p["conn"] = fill_even_odd(shape, kept)
            p["terms"] = terms[img]                       # row-major order
            p["cz"] = F(sequential_sum(p["terms"]) / p["area"])
            pieces.append(p)
    C = len(pieces)
    if C == 0 or C > 254:
        return pieces, None, None, cands
    score = np.array([F(F(p["area"] * F(0.0003)) - p["cz"]) for p in pieces], F)
    order = np.argsort(-score, kind="stable")             # order[r] = discovery index of the piece of rank r; ties: see rank_is_defined
    rank = np.empty(C, np.int64); rank[order] = np.arange(C)
    piece_of = np.full(shape, C + 1, np.uint8)
    for r, k in enumerate(order):
        piece_of[pieces[k]["img"]] = r
    for p, s in zip(pieces, score):
        p["score"] = s
    return pieces, rank, piece_of, cands


def rank_is_defined(pieces):
    """std::sort is an insertion sort up to 16 elements (stable); beyond that the order of equal scores is the implementation's, not the reference's"""
    s = [p["score"] for p in pieces]
    return len(pieces) <= 16 or len(set(float(v) for v in s)) == len(s)


def frame_ref(f):
    return seg_pieces(f.planes, f.occ1, f.edge, f.depth, f.scale)


def assert_equal_to_ref(tag, f, ref, C, recs, vals, planes, conn, piece_of, unbits):
    """one side's answer (the entries' export format, see sindh_seg_pieces) against the reference's, bit for bit"""
    pieces, rank, ref_of, _ = ref
    assert C == len(pieces), (tag, C, len(pieces))
    for i, p in enumerate(pieces[:len(recs)]):
        r = recs[i]
        got = (r[0], (r[1], r[2]), r[3], (int(r[5]) << 32) | (int(r[4]) & 0xffffffff), bool(r[6]), tuple(int(v) for v in r[7:11]))
        assert got == (p["cluster"], p["start"], p["clen"], p["sum2"], p["has_conn"], p["box"]), (tag, i, got)
        assert vals[i, 0] == p["area"] and vals[i].tobytes() == np.array([p["area"], p["cz"]], F).tobytes(), (tag, i, vals[i], p["area"], p["cz"])
        assert np.array_equal(unbits(planes[i], f.w), p["img"]), (tag, i, "piece plane")
        assert np.array_equal(unbits(conn[i], f.w), p["conn"]), (tag, i, "connection plane")
    if rank is not None and rank_is_defined(pieces):
        assert [int(r[11]) for r in recs[:C]] == [int(v) for v in rank[:len(recs)]], (tag, "rank")
        assert np.array_equal(piece_of, ref_of), (tag, "piece_of")
