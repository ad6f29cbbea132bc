"""The reference's large-motion test (oracle/dynadetect.hpp:87-99, DynaDetect.cc:1081-1114) restated in numpy, one IEEE operation at a time, and flow fields
built from prescribed magnitude multisets that put a batch ON the rule.  test_large_motion_cpu.py checks the restatement against the oracle on real frames and
that the reference alone separates both members of every pair of cases; test_large_motion_gpu.py compares the production launch with it, all by equality."""
import numpy as np

F = np.float32
INT_MIN = -2 ** 31
SIZES = [(38, 43, 64, 72), (115, 86, 192, 144), (384, 288, 640, 480)]           # fw, fh of the 0.6 grid, W, H of the frame


def _c_int(x):
    """(int) of a double the way x86 converts it (cvttsd2si): truncation; NaN, infinities and anything outside int come out as INT_MIN"""
    x = float(x)
    return int(x) if np.isfinite(x) and -2.0 ** 31 < x < 2.0 ** 31 else INT_MIN


def threshold(W, H):
    """0.3f * totalpixel, totalpixel = float(W * H) * 0.6f * 0.6f: the FULL frame's area, left to right in FP32"""
    return F(0.3) * ((F(W * H) * F(0.6)) * F(0.6))


def decide(u, v, W, H):
    """u, v: one flow field (any shape, FP32) of a W x H frame -> dict(flag, hist[256], max, endFlow, endFlow2)"""
    x = np.ascontiguousarray(u, F).ravel(); y = np.ascontiguousarray(v, F).ravel()
    with np.errstate(all="ignore"):
        xx = x * x; yy = y * y; s = xx + yy; mag = np.sqrt(s)                      # FP32 each, no contraction
        mx = F(0)
        if mag.size:
            mx = max(mx, F(mag.max()))
        a = F(np.float64(255.0) / np.float64(mx))
        r = np.rint(mag * a)                                                      # FP32 product, round half to even
    q = np.clip(np.where(np.isfinite(r), r, 0), 0, 255).astype(np.int64)          # 0 * inf (an all-zero field): NaN -> bin 0, as lrintf + saturate_cast give
    hist = np.bincount(q, minlength=256).astype(np.int32)
    with np.errstate(all="ignore"):
        end_flow = _c_int(np.float64((F(10.0) * F(0.6)) * F(255.0)) / np.float64(mx))
    ratio = F(0); thr = threshold(W, H); end_flow2 = 0
    for i in range(255):
        ratio = F(ratio + F(hist[i]))
        if ratio > thr:
            end_flow2 = i; break
    return dict(flag=int(end_flow2 > end_flow), hist=hist, max=mx, endFlow=end_flow, endFlow2=end_flow2)


# ---------------------------------------------------------------- fields on the rule
def field(fw, fh, groups, first=None, last=None):
    """A flow field of fw x fh pixels from a multiset of magnitudes: groups = [(magnitude, count), ...], the remainder of the pixels takes the last group's
    magnitude.  A magnitude m is stored as (m, 0) or (0, m) in turn, so |flow| is m exactly (sqrt(m * m) == m in binary FP without under / overflow).
    first / last: magnitude of the pixel at index 0 / n - 1 (taken out of the multiset's first group, which holds the maximum)."""
    n = fw * fh; mags = np.empty(n, F); o = 0
    for m, c in groups[:-1]:
        mags[o:o + c] = F(m); o += c
    assert o <= n, (o, n)
    mags[o:] = F(groups[-1][0])
    # spread deterministically, then pin the ends
    mags = mags[np.random.default_rng(n).permutation(n)]
    mx = mags.max(); imax = int(np.argmax(mags))
    mid = n // 2
    mags[imax], mags[mid] = mags[mid], mags[imax]                                 # the (first) maximum sits mid-field ...
    if first is not None:
        mags[0], mags[mid] = mags[mid], mags[0]                                   # ... or at the first / last index
    if last is not None:
        mags[n - 1], mags[mid] = mags[mid], mags[n - 1]
    u = np.where(np.arange(n) % 2 == 0, mags, F(0)).astype(F); v = np.where(np.arange(n) % 2 == 1, mags, F(0)).astype(F)
    assert mags.max() == mx
    return u.reshape(fh, fw), v.reshape(fh, fw)


def _bin(q, mx):
    """a magnitude that lands well inside bin q for the maximum mx"""
    return F(np.float64(q) * np.float64(mx) / 255.0)


def cases(fw, fh, W, H):
    """name -> dict(u, v, expect=(flag, endFlow, endFlow2) by design); pairs share a prefix and differ in the last word"""
    n = fw * fh; K = int(np.floor(threshold(W, H))); out = {}
    assert K + 2 < n

    def add(name, groups, expect, **kw):
        u, v = field(fw, fh, groups, **kw); out[name] = dict(u=u, v=v, expect=expect)

    # the cumulative count at bin endFlow is floor(0.3f * totalpixel) (not above the threshold: the next bin decides, flagged) or that plus one (not flagged)
    mx = F(100.0); e = 15                                                       # 1530 / 100 = 15.3
    add("count/at_floor", [(mx, 1), (_bin(e - 1, mx), 5), (_bin(e, mx), K - 5), (_bin(e + 1, mx), 0)], (1, e, e + 1))
    mx = F(99.0)                                                                # 15.45: every case has a maximum of its own (a batch must not share one)
    add("count/floor_plus_one", [(mx, 1), (_bin(e - 1, mx), 5), (_bin(e, mx), K - 4), (_bin(e + 1, mx), 0)], (0, e, e))
    # 1530 / max just above, at and just below an integer: the same counts (the threshold is passed in bin 15), endFlow 15 or 14
    m15 = F(102.0)                                                              # 1530 / 102 = 15
    for tag, m, ef in (("above", np.nextafter(m15, F(0)), 15), ("exact", m15, 15), ("below", np.nextafter(m15, F(1000)), 14)):
        add("integer/" + tag, [(m, 1), (_bin(14, m), K), (_bin(15, m), 1), (_bin(40, m), 0)], (int(15 > ef), ef, 15))
    # mag * a exactly at q + 0.5.  Max 127.5: a = 2 exactly, endFlow = 12; 6.25 -> 12.5 stays in bin 12 (even: the K + 1 pixels pass the threshold there, not
    # flagged; half away from zero would move them to bin 13: flagged).  Max 63.75: a = 4, endFlow = 24; 5.875 -> 23.5 goes up to bin 24 (odd; truncation or half
    # down would pass the threshold in bin 23).  Max 255: a = 1, endFlow = 6; 7.5 goes up to bin 8: flagged
    add("half/even", [(F(127.5), 1), (F(6.25), K + 1), (F(20.0), 0)], (0, 12, 12))
    add("half/odd", [(F(63.75), 1), (F(5.875), K + 1), (F(20.0), 0)], (0, 24, 24))
    add("half/odd_up", [(F(255.0), 1), (F(7.5), K + 1), (F(20.0), 0)], (1, 6, 8))
    # the maximum at the first / at the last index only
    add("ends/first", [(F(60.0), 1), (_bin(25, F(60.0)), K), (_bin(26, F(60.0)), 0)], (1, 25, 26), first=True)
    add("ends/last", [(F(61.0), 1), (_bin(25, F(61.0)), K + 1), (_bin(26, F(61.0)), 0)], (0, 25, 25), last=True)
    # tiny and huge magnitudes: 1530 / 1e-20 does not fit an int (the conversion gives INT_MIN: flagged whatever the histogram), m * m is subnormal;
    # 1530 / 3e6 -> endFlow 0
    mt = F(1e-20)
    add("range/tiny", [(mt, 1), (_bin(3, mt), K + 1), (_bin(200, mt), 0)], None)
    mb = F(3e6)
    add("range/huge_flagged", [(mb, 1), (_bin(0, mb), K), (_bin(7, mb), 0)], (1, 0, 7))
    add("range/huge_calm", [(mb, 1), (F(0.0), K + 1), (_bin(7, mb), 0)], (0, 0, 0))
    # a static pair: zero flow everywhere -> the maximum is 0, a = inf, every pixel in bin 0, endFlow = (int)inf: flagged, as the oracle does on static frames
    out["zero"] = dict(u=np.zeros((fh, fw), F), v=np.zeros((fh, fw), F), expect=(1, INT_MIN, 0))
    # general position: both components non-zero (the rounding of x * x + y * y), a smooth field plus noise
    rng = np.random.default_rng(fw * 1000 + fh)
    yy, xx = np.mgrid[0:fh, 0:fw]
    u = (0.02 * xx + rng.standard_normal((fh, fw))).astype(F); v = (0.5 - 0.01 * yy + 0.3 * rng.standard_normal((fh, fw))).astype(F)
    out["general/calm"] = dict(u=u, v=v, expect=None)
    out["general/fast"] = dict(u=(u * F(9.0) + F(11.0)).astype(F), v=(v * F(7.0)).astype(F), expect=None)
    return out


PAIRS = [("count/at_floor", "count/floor_plus_one"), ("integer/below", "integer/above"), ("integer/below", "integer/exact"), ("half/odd_up", "half/even"),
         ("ends/first", "ends/last"), ("range/huge_flagged", "range/huge_calm")]            # (flagged, not flagged)


def batches(names, B):
    """batches of B case names: every case appears, the image with the largest maximum (range/huge_*) is neither first nor last, and every batch of B >= 3
    holds the all-zero image"""
    if B == 1:
        return [[n] for n in names]
    rest = [n for n in names if n not in ("zero", "range/huge_flagged", "range/huge_calm")]
    out = []; per = B - 2
    for i in range(0, len(rest), per):
        part = rest[i:i + per]
        while len(part) < per:
            part.append(rest[(i + len(part)) % len(rest)])
        # (the all-zero image is flagged, the huge calm one is not: every batch holds both flags)
        out.append(["zero", "range/huge_calm"] + part[::-1] if len(out) % 2 else [part[0], "range/huge_calm"] + part[1:] + ["zero"])
    out.append(["zero", "range/huge_flagged", "count/floor_plus_one", "half/even", "integer/above"][:B])
    return out
