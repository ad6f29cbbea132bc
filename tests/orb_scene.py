"""Deterministic inputs for the ORB extractor tests (numpy only, seeded): image content that drives each branch of the extractor, the
image geometries the suite pins, and a mask builder that leaves an exact number of keypoints outside the dynamic area."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------- content
def tex(w, h, seed=0):
    """6 x 6 blocks of random grey plus +-8 noise: corners at every strength, on every level"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (h // 6 + 2, w // 6 + 2))
    img = np.kron(g, np.ones((6, 6), np.int64))[:h, :w] + rng.integers(-8, 9, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def binary_blocks(w, h, seed=0):
    """saturated 7 x 5 checkerboard: FAST scores reach 254, plateaus of equal scores meet the strict-maximum NMS, and hundreds of
    orientations land exactly on 0 / 90 / 180 / 270 degrees"""
    yy, xx = np.mgrid[:h, :w]
    return (((xx // 7 + yy // 5) % 2) * 255).astype(np.uint8)


def binary_noise(w, h, seed=0):
    return ((np.random.default_rng(seed).random((h, w)) < 0.5) * 255).astype(np.uint8)


def low_contrast(w, h, seed=0):
    """steps of 12 grey levels: nothing passes an initial threshold of 20, every cell takes the second pass"""
    yy, xx = np.mgrid[:h, :w]
    return (100 + ((xx // 9 + yy // 9) % 2) * 12 + np.random.default_rng(seed).integers(0, 2, (h, w))).astype(np.uint8)


def dots(w, h, seed=0):
    yy, xx = np.mgrid[:h, :w]
    return (((xx % 40 == 20) & (yy % 40 == 20)) * 255).astype(np.uint8)


def half_flat(w, h, seed=0):
    img = tex(w, h, seed); img[:, : w // 2] = 77
    return img


def mixed_contrast(w, h, seed=0):
    """full-contrast texture above, the same kind squeezed into 14 grey levels below: some cells are decided by the first FAST pass,
    others by the retry"""
    img = tex(w, h, 2)
    img[h // 2:] = (100 + tex(w, h, 4).astype(np.int64) * 14 // 255).astype(np.uint8)[h // 2:]
    return img


CONTENT = {"binary_blocks": binary_blocks, "binary_noise": binary_noise, "low_contrast": low_contrast, "dots": dots,
           "half_flat": half_flat, "mixed_contrast": mixed_contrast}

# ---------------------------------------------------------------------------------------------------------------- geometry
NFEATURES = 1500
# (width, height, scaleFactor, nlevels)
GEOMETRY = [
    (641, 479, 1.2, 8),     # odd width and height
    (223, 223, 1.2, 8),     # last level is 62 x 62, the smallest that holds a cell
    (250, 130, 1.2, 4),     # small, wide
    (91, 91, 1.2, 1),       # one level; its single cell is the 59 x 59 window, the largest a cell can be
    (322, 246, 2.0, 3),     # scale factor 2.0
    (515, 389, 1.1, 12),    # scale factor 1.1, 12 levels
    (1000, 260, 1.2, 6),    # nearly 4:1, four initial octree nodes
    (129, 127, 1.5, 2),     # scale factor 1.5
    (752, 480, 1.2, 8),     # another common sensor size
    (64, 64, 1.2, 1),       # the minimum size
    (150, 120, 1.2, 8),     # the top four levels are 72 x 58 down to 42 x 33 and hold no cell
    (480, 640, 1.2, 8),     # portrait inside the domain
]


def level_sizes(w, h, scale_factor, nlevels):
    """(width, height) of every pyramid level, in the extractor's FP32 arithmetic (ORBextractor.cc:418-431, :1170-1171)"""
    f32 = np.float32
    sc = [f32(1)]
    for _ in range(1, nlevels):
        sc.append(f32(np.float64(sc[-1]) * np.float64(f32(scale_factor))))
    out = []
    for s in sc:
        inv = f32(1) / s
        out.append((int(np.rint(f32(w) * inv)), int(np.rint(f32(h) * inv))))
    return out


def holds_cell(lw, lh):
    """a level has FAST cells when its bordered extent (16 px off each side) fits one 30-px cell both ways"""
    return lw - 32 >= 30 and lh - 32 >= 30


def oracle_can_take(w, h, scale_factor, nlevels):
    """False where the oracle (and the reference) is undefined: a level exactly 32 px wide or high (0 / 0 in DistributeOctTree), or a
    level with cells whose bordered width / height rounds to zero initial nodes"""
    for lw, lh in level_sizes(w, h, scale_factor, nlevels):
        if lw == 32 or lh == 32:
            return False
        if holds_cell(lw, lh) and np.round(np.float32(lw - 32) / np.float32(lh - 32)) < 1:
            return False
    return True


def geometry_mask(w, h):
    """dynamic (255) on the left 40 % of the columns, plus a block of 254 that must NOT count as dynamic"""
    m = np.zeros((h, w), np.uint8)
    m[:, : int(w * 0.4)] = 255
    m[h // 4: h // 2, w // 2: 3 * w // 4] = 254
    return m


# ---------------------------------------------------------------------------------------------------------------- masks
def lookup_pixels(selected, scale_factor):
    """the mask pixel (row, col) the extractor reads for each octree survivor (level coordinates, octave set):
    (int(y * s), int(x * s)) with s = float(pow(double(scaleFactor), octave)), products in FP32 (ORBextractor.cc:1078-1080)"""
    s = np.power(np.float64(np.float32(scale_factor)), selected["octave"].astype(np.float64)).astype(np.float32)
    return (selected["y"] * s).astype(np.int64), (selected["x"] * s).astype(np.int64)


def mask_leaving(oracle_selected_per_level, scale_factor, keep_n, shape):
    """An all-255 mask with 254 at the lookup pixels of exactly keep_n survivors.  Keypoints of different octaves can share a lookup
    pixel, so pixels are opened group by group and a group that would overshoot is skipped.  Returns (mask, survivors achieved)."""
    sel = np.concatenate(list(oracle_selected_per_level))
    r, c = lookup_pixels(sel, scale_factor)
    groups = {}
    for p in zip(r.tolist(), c.tolist()):
        groups[p] = groups.get(p, 0) + 1
    mask = np.full(shape, 255, np.uint8); n = 0
    for (pr, pc), cnt in groups.items():
        if n + cnt > keep_n:
            continue
        mask[pr, pc] = 254; n += cnt
        if n == keep_n:
            break
    return mask, n
