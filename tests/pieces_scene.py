"""Crafted scenes for the piece extraction of SegAndMerge: bit planes for the border following, and frames (cluster planes, occlusion edges, edge clusters, depth)
for the whole stage.  Every scene is made for one rule; the tests assert that rule from the numpy reference's own record before they compare anything.

The piece stage follows borders twice: on the clusters after their 4 x 4 opening, where no row run is shorter than two pixels, and on the thin band planes of the
second level.  One-pixel lines, single pixels, checkerboards and thin walls therefore reach the border following only through the contour entry points
(sindh_find_contours, sind_debug_contours) and through the second level; the contour scenes below are for the former."""
import numpy as np

CONTOUR_SIZES = [(64, 64), (128, 72), (192, 136)]          # (w, h); 64: one word per row
CONTOUR_CAPS = (1024, 32768)                               # the documented capacities: contours and chain points per plane (pieces_dev.hpp)


def bits(m):
    """bool [h][w] -> the library's bit planes: [h][ceil(w / 64)] words, bit x & 63 of word x / 64"""
    h, w = m.shape; wpr = (w + 63) // 64
    p = np.zeros((h, wpr * 64), np.uint8); p[:, :w] = m
    return np.ascontiguousarray(np.packbits(p, axis=1, bitorder="little")).view("<u8").reshape(h, wpr)


def unbits(words, w):
    h, wpr = words.shape
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(h, wpr, 8), axis=-1, bitorder="little").reshape(h, wpr * 64)
    return b[:, :w].astype(bool)


def contour_scenes(w, h):
    """name -> bool [h][w]"""
    z = lambda: np.zeros((h, w), bool)
    s = {}
    s["empty"] = z()
    s["full"] = ~z()
    m = z(); m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = m[h // 2, w // 2] = m[5, 9] = True; s["single_pixels"] = m
    m = z(); m[7, 3:w - 5] = True; s["line_horizontal"] = m
    m = z(); m[2:h - 3, 11] = True; s["line_vertical"] = m
    m = z(); n = min(w, h) - 4; m[np.arange(n) + 2, np.arange(n) + 1] = True; s["line_diagonal"] = m
    m = z(); n = min(w, h) - 4; m[np.arange(n) + 2, w - 2 - np.arange(n)] = True; s["line_antidiagonal"] = m
    m = z()
    m[0:5, 0:6] = m[0:4, w - 7:w] = m[h - 6:h, 0:4] = m[h - 3:h, w - 5:w] = True                                        # the corners
    m[0:3, w // 2 - 4:w // 2 + 4] = m[h - 4:h, w // 2 - 3:w // 2 + 5] = m[h // 2 - 3:h // 2 + 3, 0:3] = m[h // 2 - 2:h // 2 + 4, w - 4:w] = True      # the sides
    s["border_blobs"] = m
    m = z(); m[10:14, 50:64] = True                                                                                      # a run that ends at bit 63
    if w > 64:
        m[20:23, 64:75] = True; m[30:33, 60:70] = True                                                                   # one that starts at bit 64, one that crosses
    s["word_seams"] = m
    m = z(); m[8:30, 8:40] = True; m[13:25, 14:34] = False; m[17:21, 20:28] = True; s["hole_and_island"] = m             # the island inside the hole is not reported
    m = z(); m[8:24, 8:30] = True; m[10:22, 9:20] = False; s["hole_behind_thin_wall"] = m                                # the wall left of the hole is one pixel wide
    m = z(); m[5:10, 5:10] = True; m[10:15, 10:15] = True; m[15:20, 5:10] = True; m[30:33, 30:33] = True; m[33:36, 27:30] = True; s["diagonal_touch"] = m
    m = z(); yy, xx = np.mgrid[0:8, 0:8]; m[20:28, 12:20] = (yy + xx) % 2 == 0; s["checkerboard"] = m
    step = {64: 3, 128: 4, 192: 6}[w]
    m = z(); m[1::step, 1::step] = True; s["many_components"] = m
    m = z(); m[h - 3:h - 1, 2:w - 2] = True; m[2:h - 3, 2:w - 2:2] = True; s["comb"] = m                          # one chain of several thousand points
    return s


OVERFLOW = {"many_components": (10, 32768, 1), "comb": (1024, 400, 2)}          # scene -> (cap_contours, cap_points, the status the device reports)


# ---------------------------------------------------------------------------------------------------------------- frames for the whole stage
# Shapes whose contour AFTER the 4 x 4 opening sits on a rule (found by search with the oracle; the tests assert the figures from the reference's record):
#   tall(a, b): an a x b rectangle; ear(a, b, ea, eb, off): the same with an ea x eb ear on its right side, off rows below the top
def tall(m, x, y, a, b):
    m[y:y + b, x:x + a] = True


def ear(m, x, y, a, b, ea, eb, off):
    m[y:y + b, x:x + a] = True; m[y + off:y + off + eb, x + a:x + a + ea] = True


class Frame:
    def __init__(self, w, h, k=1, depth=5000, scale=5000.0):
        self.w, self.h, self.scale = w, h, float(scale)
        self.planes = np.zeros((k, h, w), bool); self.occ1 = np.zeros((h, w), bool); self.edge = np.ones((h, w), bool)
        self.depth = np.full((h, w), depth, np.uint16)


def z_invalid_from(scale):
    d = np.arange(65536, dtype=np.float32) / np.float32(scale)
    bad = np.nonzero(d >= np.float32(6))[0]
    return int(bad[0]) if len(bad) else 65536


def piece_scenes():
    """name -> Frame"""
    s = {}
    f = Frame(192, 136); tall(f.planes[0], 10, 10, 6, 22); tall(f.planes[0], 40, 10, 6, 23); f.planes[0][10, 40:43] = False; s["length_50_51"] = f
    f = Frame(192, 136); ear(f.planes[0], 10, 10, 4, 18, 8, 5, 0); ear(f.planes[0], 40, 10, 4, 19, 7, 5, 1); ear(f.planes[0], 70, 10, 4, 21, 6, 5, 0); s["area_160_161_162"] = f
    f = Frame(192, 136); tall(f.planes[0], 10, 10, 4, 25); tall(f.planes[0], 40, 10, 13, 13); s["thin_and_square"] = f          # length passes / area fails, area passes / length fails: no piece
    f = Frame(192, 136, k=2); f.planes[0][20:70, 20:80] = True; f.planes[0][35:55, 35:65] = False; f.planes[1][35:55, 35:65] = True
    f.planes[1][41:49, 44:56] = False; f.planes[0][41:49, 44:56] = True; s["hole_and_island"] = f          # the fill closes the hole, the cluster plane opens it again; the island joins
    f = Frame(192, 136); f.planes[0][20:80, 20:100] = True; f.occ1[20:80, 58:61] = True; s["occ_cuts_a_cluster"] = f
    f = Frame(192, 136); f.planes[0][30:70, 20:60] = True; f.planes[0][30:70, 100:140] = True; f.edge[:] = False
    f.edge[30:33, 30:37] = True; f.edge[30:33, 110:117] = True; f.edge[30, 110] = False; s["band_20_21"] = f
    f = Frame(192, 136); f.planes[0][30:70, 20:60] = True; f.planes[0][30:70, 100:140] = True; f.edge[:] = False
    f.edge[30:33, 30:44] = True; f.edge[30:33, 110:124] = True; f.edge[30, 110] = False; s["second_level_29_30"] = f
    f = Frame(192, 136); f.planes[0][30:90, 20:120] = True; f.edge[:] = False
    f.edge[30:33, 30:50] = True; f.edge[30:33, 70:90] = True; f.edge[60:75, 20:23] = True; s["two_kept_contours"] = f          # three kept borders on one piece, drawn into one plane
    f = Frame(192, 136, depth=0); f.planes[0][30:70, 20:60] = True; s["no_valid_depth"] = f
    for scale in (5000.0, 1000.0):
        zi = z_invalid_from(scale)
        f = Frame(192, 136, depth=900, scale=scale); f.planes[0][30:70, 20:60] = True
        f.depth[40, 25:30] = 0; f.depth[41, 25:30] = min(zi, 65535); f.depth[42, 25:30] = zi - 1; f.depth[43, 25:30] = 65535; s["depth_limits_%d" % int(scale)] = f
    f = Frame(192, 136); f.planes[0][20:90, 20:120] = True; f.depth[:] = np.random.RandomState(3).randint(400, 29000, f.depth.shape); s["sequential_sum"] = f
    f = Frame(192, 136, k=2); f.planes[0][30:70, 20:60] = True; f.planes[1][30:70, 100:140] = True; s["score_tie"] = f
    f = Frame(192, 136, k=3); s["no_pieces"] = f
    f = Frame(192, 136, k=3)
    for i in range(3):
        for q in range(8):
            tall(f.planes[i], 6 + 22 * q, 6 + 42 * i, 8 + q, 30 + i)
    f.depth[:] = (np.arange(136)[:, None] * 40 + np.arange(192)[None, :] * 7 + 600).astype(np.uint16); f.occ1[60:63, :] = True; s["crowded"] = f
    f = Frame(192, 136, k=4); r = np.random.RandomState(11)
    for i in range(4):
        for _ in range(3):
            x, y = r.randint(0, 150), r.randint(0, 100); f.planes[i][y:y + r.randint(12, 36), x:x + r.randint(12, 40)] = True
    for i in range(1, 4):
        f.planes[i] &= ~f.planes[:i].any(axis=0)
    f.occ1[:, 95:97] = True; f.edge = f.planes[:2].any(axis=0); f.depth[:] = r.randint(300, 40000, f.depth.shape); s["ordinary"] = f
    return s


def too_many_pieces():
    f = Frame(384, 288)
    for y in range(4, 288 - 26, 28):
        for x in range(4, 384 - 8, 10):
            tall(f.planes[0], x, y, 6, 24)
    return f


def chain_overflow():
    """640 x 480: a comb whose teeth survive the opening; its one contour has more points than a plane's chain holds"""
    f = Frame(640, 480); f.planes[0][470:476, 4:636] = True
    for x in range(4, 632, 8):
        f.planes[0][4:470, x:x + 4] = True
    return f


def synthetic_frame():
    """640 x 480 from the synthetic stream: its depth cut into six bands as the cluster planes, its depth steps as the occlusion edges"""
    from sindslam_amd.synth import SyntheticStream
    _, depth = SyntheticStream().frames(0, 1)
    d = np.ascontiguousarray(depth[0]); f = Frame(640, 480, k=6, scale=5000.0); f.depth = d
    valid = d > 0; qs = np.quantile(d[valid], np.linspace(0, 1, 7)); qs[-1] += 1
    for i in range(6):
        f.planes[i] = valid & (d >= qs[i]) & (d < qs[i + 1])
    g = np.zeros(d.shape, bool); di = d.astype(np.int32)
    g[:, 1:] |= np.abs(di[:, 1:] - di[:, :-1]) > 400; g[1:, :] |= np.abs(di[1:, :] - di[:-1, :]) > 400
    f.occ1 = g; f.edge = f.planes[:3].any(axis=0)
    return f
