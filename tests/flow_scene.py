"""Scene makers for the flow tests on sparse, flat, static and saturated content (tests/test_flow_sparse_cpu.py, tests/test_flow_sparse_gpu.py).

The other flow tests feed the kernels a band-limited random texture with an initial flow drawn from N(0, 1): no exact zero, no denormal, no saturated plateau and no
rounding tie is ever in flight.  The scenes here put exactly those in flight; all are deterministic functions of their arguments."""
import numpy as np

# DeepFlow's level parameters in float32 arithmetic as in deepflow.cpp (4 * alpha, delta / 3, gamma / 3), omega 1.6
DEEPFLOW_LEVEL = (4 * np.float32(1.0), np.float32(0.5) / np.float32(3), np.float32(5.0) / np.float32(3), 1.6)

# (seed, w, h, cw, fixed-point iterations, SOR iterations) of every sparse scene the GPU tests solve; tests/test_flow_sparse_cpu.py asserts that the oracle's own run reaches
# the sub-2^-116 and the denormal range on each of them
SPARSE_SOLVER_SCENES = [(45, 300, 33, 16, 1, 100), (46, 300, 33, 16, 1, 100), (4, 300, 33, 16, 1, 100), (0, 385, 35, 16, 5, 25)]
# the same content at 384 columns, the widest level of the 384 x 288 handle that tests/test_flow_coarse_gpu.py takes through k_sor_tile
SPARSE_TILE_SCENES = SPARSE_SOLVER_SCENES[:3] + [(0, 384, 35, 16, 5, 25)]
# one workgroup's level (k_coarse_chain: at most 120 columns at 33 rows) with a flat run of 112 / 116 pixels.  After 100 SOR iterations the increment 112 pixels from the strip
# is still 2^-46: the front has had time to fill in.  FEWER iterations leave it steeper -- after 50 (1 x 50, 5 x 10) the last columns are denormal, after 40 still zero.
SPARSE_CHAIN_SCENES = [(45, 120, 33, 8, 1, 50), (45, 120, 33, 4, 5, 10)]


def sparse_strip(seed, w, h, cw=16):
    """a flat field of 128 with a strip of cw columns of white noise on the left, and the same with the strip rolled down by one row: the solver's increment spreads from the
    strip into the flat field one pixel per half-sweep and loses about 1.4 binary orders per pixel -- far from the strip it is below 2^-105, then denormal, then zero"""
    rng = np.random.default_rng(seed)
    i0 = np.full((h, w), 128, np.float32)
    tex = rng.integers(0, 256, (h, cw))
    i0[:, :cw] = tex
    i1 = i0.copy(); i1[:, :cw] = np.roll(tex, 1, 0)
    return i0, i1


def textured(w, h, seed, dx=3, dy=-2):
    """a band-limited random texture and a copy shifted by (dx, dy) pixels, integer values 0 .. 255 as float32 (the texture of tests/test_flow_gpu.py)"""
    rng = np.random.default_rng(seed)
    base = rng.normal(0, 1, (h + 16, w + 16)).astype(np.float32)
    for _ in range(3):
        base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) * np.float32(0.25)
    base = (base - base.min()) / (base.max() - base.min()) * np.float32(255)
    return np.rint(base[8:8 + h, 8:8 + w]).astype(np.float32), np.rint(base[8 + dy:8 + dy + h, 8 + dx:8 + dx + w]).astype(np.float32)


def flat(v, w, h):
    """two identical constant images"""
    a = np.full((h, w), v, np.uint8)
    return a, a.copy()


def static_pair(w, h, seed):
    """a textured image and itself (i1 is i0)"""
    a = textured(w, h, seed)[0].astype(np.uint8)
    return a, a


def plateau(w, h, seed, value):
    """a textured pair whose right half is one plateau of `value` (255: saturated, 0: black) in both images: the texture moves, the plateau and its edge do not"""
    a, b = textured(w, h, seed)
    a = a.astype(np.uint8); b = b.astype(np.uint8)
    a[:, w // 2:] = value; b[:, w // 2:] = value
    return a, b


def blob_on_flat(w, h):
    """a 20 x 20 square of 200 on 128, and the same shifted right by one pixel"""
    a = np.full((h, w), 128, np.uint8); b = a.copy()
    y, x = h // 2 - 10, w // 2 - 10
    a[y:y + 20, x:x + 20] = 200; b[y:y + 20, x + 1:x + 21] = 200
    return a, b


def tie_flow(w, h, seed):
    """an initial flow (u, v) whose every value is an odd multiple of 1/64 within +- 2 max(w, h): (x + u) * 32 is an exact .5 tie for the warp's cvRound, and the warped
    positions reach well outside the frame on every side (still inside the +- 32768 clamp).  The four corners are pinned outside: left / above, right / below."""
    rng = np.random.default_rng(seed)
    m = 2 * max(w, h)
    u = ((2 * rng.integers(-32 * m, 32 * m, (h, w)) + 1) / 64).astype(np.float32)
    v = ((2 * rng.integers(-32 * m, 32 * m, (h, w)) + 1) / 64).astype(np.float32)
    far = np.float32(m - 1 / 64)
    u[0, 0] = -far; v[0, 0] = -far; u[-1, -1] = far; v[-1, -1] = far
    u[0, -1] = far; v[0, -1] = -far; u[-1, 0] = -far; v[-1, 0] = far
    return u, v


def half_saturated(bgr):
    """frames with columns 320 and up set to 255 in every channel"""
    out = np.array(bgr, copy=True); out[..., 320:, :] = 255
    return out


def count_tiny(a):
    """(non-zero values below 2^-116, denormals) of a float32 plane"""
    m = np.abs(a.astype(np.float64))
    return int(((m > 0) & (m < 2.0 ** -116)).sum()), int(((m > 0) & (m < 2.0 ** -126)).sum())
