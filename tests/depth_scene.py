"""Deterministic hostile depth content for the depth half of DynaDetect (numpy only).  TEST INFRASTRUCTURE ONLY.

front_frames(w, h)      single frames for the front of CalOccluded and the depth normalisation, each built so that the 5 x 5 median does not move what it
                        carries: column-constant plateaus at least 8 px wide and column-constant ramps are fixed points of the median
front_batches(w, h)     triples of those frames whose members differ from each other (per-frame maxima slots, frame offsets)
rewrite(kind, depth)    the depth of a SyntheticStream frame rewritten for the whole-detector tests
"""
import functools

import numpy as np

FRONT_SIZES = [(64, 64), (128, 72), (192, 136), (71, 13)]
# depth scales of the 6 m ramps: two round ones, two that are not, and three found by search where the rounding of the FP32 quotient decides: at 1006 and 3400 the
# product d * (1 / depthScale) for d = 6 * depthScale rounds BELOW 6 while the division gives exactly 6 (invalid); at 5000 + 683 / 2048 the raw value 30002 lies 0.00098 under
# 6 * depthScale and the FP32 quotient rounds UP to 6.0f (invalid), where exact or FP64 arithmetic calls the pixel valid
SCALES_6M = [5000.0, 1000.0, 5208.0, 999.9, 1006.0, 3400.0, 5000.33349609375]
KINDS = ["plain", "speckle", "saturated", "steps", "border", "lowrange"]
# (width, height, intrinsics, base of the `steps` kind): 192 x 136 grows the PEAC regions on the host, 192 x 144 in the kernel; steps from 5000 lie beyond 6 m at the D455 factor 1000
CONTENT_SIZES = [(192, 136, "TUM3", 5000), (192, 144, "TUM3", 5000), (256, 192, "D455", 1000), (320, 240, "TUM3", 5000)]
SMALL_PLAIN = [(64, 64), (128, 72)]            # the detector runs, but finds no plane and nothing dynamic


def _bands(w, h, levels):
    """column-constant image of 8-px bands (the last level fills the rest of the row)"""
    idx = np.minimum(np.arange(w) // 8, len(levels) - 1)
    return np.broadcast_to(np.asarray(levels, np.int64)[idx], (h, w)).astype(np.uint16)


def ties_400(w, h):
    """neighbouring plateaus exactly 400 and 401 apart, rising and falling: val_max == 400 is no edge, 401 is one"""
    steps = [400, 401, -400, -401, 401, 400, -401]
    return _bands(w, h, np.concatenate([[5000], 5000 + np.cumsum(steps)]))


def ties_3pct(w, h):
    """depth1 = 20000 beside plateaus 600 and 601 away: 20000 * 0.03f rounds to 600.0f, so 600 is no edge and 601 is one"""
    return _bands(w, h, [20000, 20600, 20000, 20601, 20000, 19400, 20000, 19399])


def ties_half(w, h, dmax):
    """depth1 - nb on both sides of depth_max * 0.5f (a neighbour beyond it is skipped): dmax even -> the difference equals the half and exceeds it by one,
    dmax odd -> the half ends in .5 and the differences lie half a unit on either side"""
    lo = dmax - dmax // 2                      # dmax - lo == floor(dmax / 2)
    return _bands(w, h, [dmax, lo, dmax, lo - 1, dmax, lo, lo - 1, dmax])


def ramp_6m(w, h, depth_scale, shift=0):
    """d[y, x] = base + x around 6 * depth_scale: the pixels on both sides of depth1 / depthScale < 6.0f, to half the width on either side"""
    base = int(round(6 * depth_scale)) - w // 2 + shift
    return np.broadcast_to(base + np.arange(w), (h, w)).astype(np.uint16)


def salt_pepper(w, h, seed=11):
    """a slanted plane with 30 % of the pixels drawn from {0, 1, 32768, 65535}; the four corners always, and at least one pixel of every border line"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (5000 + 3 * xx + 2 * yy).astype(np.uint16)
    vals = np.array([0, 1, 32768, 65535], np.uint16)
    hit = rng.random((h, w)) < 0.30
    d[hit] = vals[rng.integers(0, 4, int(hit.sum()))]
    d[0, 0], d[0, -1], d[-1, 0], d[-1, -1] = 65535, 0, 1, 32768
    d[0, w // 2], d[-1, w // 2], d[h // 2, 0], d[h // 2, -1] = 32768, 65535, 0, 1
    return d


def max_at(w, h, last):
    """the raw maximum (50001) at the first / last pixel only, and the maximum of the median-filtered frame (50000) there only: the corner pixel and its two
    neighbours weigh 15 of the 25 replicated-border samples of the corner's window and at most 11 of any other window"""
    d = np.full((h, w), 1000, np.uint16)
    d[0, 0] = 50001; d[0, 1] = d[1, 0] = 50000
    return np.ascontiguousarray(d[::-1, ::-1]) if last else d


def norm_frame(w, h, dmax):
    """every value 0 .. dmax (as far as the frame has pixels), the maximum once, at an inner pixel"""
    yy, xx = np.mgrid[0:h, 0:w]
    if dmax == 0:
        return np.zeros((h, w), np.uint16)
    if dmax <= 1024:
        d = ((xx + yy * w) % dmax).astype(np.uint16)             # 0 .. dmax - 1
    else:
        d = ((xx * 1021 + yy * 7919) % dmax).astype(np.uint16)
    d[h // 2, w // 3] = dmax
    return d


def front_frames(w, h):
    """name -> (frame, depth_scale)"""
    f = dict(ties_400=(ties_400(w, h), 5000.0), ties_3pct=(ties_3pct(w, h), 5000.0), half_even=(ties_half(w, h, 40000), 5000.0), half_odd=(ties_half(w, h, 40001), 5000.0),
             salt_pepper=(salt_pepper(w, h), 5000.0), max_first=(max_at(w, h, False), 5000.0), max_last=(max_at(w, h, True), 5000.0),
             norm_510=(norm_frame(w, h, 510), 5000.0), norm_65535=(norm_frame(w, h, 65535), 5000.0), norm_1=(norm_frame(w, h, 1), 5000.0), zero=(norm_frame(w, h, 0), 5000.0))
    for ds in SCALES_6M:
        f[f"ramp_{ds:g}"] = (ramp_6m(w, h, ds), ds); f[f"ramp1_{ds:g}"] = (ramp_6m(w, h, ds, 1), ds)
    return f


def front_batches(w, h):
    """[(names, depth_scale)]: three different frames per launch; [bright, all zero, dim] shows a maximum that leaks between the per-frame slots"""
    b = [(("salt_pepper", "zero", "norm_510"), 5000.0), (("max_first", "zero", "norm_1"), 5000.0), (("ties_400", "ties_3pct", "half_even"), 5000.0),
         (("half_odd", "max_last", "norm_65535"), 5000.0)]
    for ds in SCALES_6M:
        b.append(((f"ramp_{ds:g}", "zero", f"ramp1_{ds:g}"), ds))
    return b


# ---------------------------------------------------------------- whole-detector content
def rewrite(kind, depth, seed=5, steps_base=5000):
    """the depth frame of a stream rewritten; `depth` is not changed"""
    d = np.array(depth, np.uint16, copy=True); h, w = d.shape
    if kind == "plain":
        return d
    if kind == "speckle":                      # single pixels, not aligned to anything: 0.1 % holes, 0.05 % saturated
        rng = np.random.default_rng(seed + 7 * w + h)
        r = rng.random((h, w))
        d[r < 0.001] = 0; d[(r >= 0.001) & (r < 0.0015)] = 65535
        return d
    if kind == "saturated":                    # a quarter of the frame and the top three rows / right three columns at the top of the range
        d[h // 4:h // 4 + h // 2, w // 4:w // 4 + w // 2] = 65535
        d[:3, :] = 65535; d[:, -3:] = 65535
        return d
    if kind == "steps":                        # 16-px plateaus 400 apart along x and 401 along y, every (7th row, 5th column) pixel one higher
        yy, xx = np.mgrid[0:h, 0:w]
        s = steps_base + 400 * (xx // 16) + 401 * (yy // 16)
        s[::7, ::5] += 1
        return s.astype(np.uint16)
    if kind == "border":                       # nothing in the outer three rows / columns, then a row near the top of the range and a column at 1
        d[3, :] = 60000; d[-4, :] = 60000; d[:, 3] = 1; d[:, -4] = 1
        d[:3, :] = 0; d[-3:, :] = 0; d[:, :3] = 0; d[:, -3:] = 0
        return d
    if kind == "lowrange":                     # the whole frame rescaled to 0 .. 510: every odd value ties in the 8-bit normalisation
        m = int(d.max())
        return ((d.astype(np.uint32) * 510 + m // 2) // m).astype(np.uint16)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _stream_frames(width, height, intr_name, count):
    import sindslam_amd.synth as synth
    s = synth.SyntheticStream(width, height, seed=3, intr=getattr(synth, intr_name))
    bgr, depth = s.frames(0, count)
    bgr.setflags(write=False); depth.setflags(write=False)
    return bgr, depth, (s.fx, s.fy, s.cx, s.cy, getattr(synth, intr_name)["depth_factor"])


def stream_case(width, height, kind, intr="TUM3", steps_base=5000, count=4):
    """(bgr [count], depth [count] rewritten, K) of SyntheticStream(width, height, seed=3, intr); intr names a set of intrinsics of sindslam_amd.synth"""
    bgr, depth, K = _stream_frames(width, height, intr, count)
    dd = np.stack([rewrite(kind, depth[t], seed=6 + t, steps_base=steps_base) for t in range(count)])
    return bgr, dd, K
