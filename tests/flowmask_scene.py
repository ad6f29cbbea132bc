"""Scenes for the flow-mask stage that sit on its rules (u8 rounding ties, where the maximum lies, the branch between Otsu and Triangle, every clamp comparison with
the constant quotient equal to the threshold and one ulp to either side, the count rule, Otsu's and Triangle's ties, the mask comparison, a non-trivial homography).

Two builders.  field_from_bins makes a flow field from a wanted bin per pixel and a maximum M: the homography is the identity and v = 0, so the residual is |u|
exactly, the pixel of bin b holds a float near b / a (a = float32(255 / M)) and exactly one pixel holds M.  block makes a (histogram, M) block for the threshold
entry directly.  Every scene carries the property it was built for (`prop`, a sentence, and `holds`, a predicate on the numpy reference's result): the CPU test
asserts it, so a scene cannot pass for the wrong reason.  Histograms with wanted Otsu / Triangle values are searched for in a fixed family with the reference.

Out of scope: non-finite flow or homography, and a denominator that crosses zero inside the image (the flow solvers are pinned to finite output, and
findHomography normalises H[8] to 1)."""
import numpy as np

import flowmask_ref as R

f32 = np.float32
f64 = np.float64
EYE = np.eye(3).ravel()
SIZES = [(64, 1), (64, 8), (192, 13), (128, 24)]
BLOCK_SIZES = SIZES + [(384, 288), (640, 480), (1280, 720), (1920, 1080)]


class Scene:
    """a field scene (u, v, H) or a block scene (hist, M); prop / holds: the property it was built for"""

    def __init__(self, name, prop, holds, W, H, u=None, v=None, Hm=None, hist=None, M=None):
        self.name, self.prop, self.holds, self.W, self.H = name, prop, holds, W, H
        self.u, self.v, self.Hm, self.hist, self.M = u, v, Hm, hist, M

    def __repr__(self):
        return self.name

    def ref(self):
        """the numpy reference's result for this scene, computed once"""
        if not hasattr(self, "_ref"):
            if self.u is not None:
                self._ref = R.stage(self.u, self.v, self.Hm)
            else:
                self._ref = R.thresholds(self.hist, self.W, self.H, self.M); self._ref.update(hist=self.hist, maxError=self.M)
        return self._ref


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def down(x):
    return np.nextafter(f32(x), f32(-np.inf))


# ---------------------------------------------------------------------------------------------------------------- builders
def bin_values(M):
    """256 floats: value b lands in bin b under the maximum M (and lies below M)"""
    M = f32(M); a = f32(f64(255.0) / f64(M)); out = np.zeros(256, f32)
    for b in range(256):
        x = f32(f64(b if b < 255 else 254.75) / f64(a))
        for _ in range(8):                                 # a float near b / a; nudged if the product rounds into the neighbour
            q = np.rint(x * a)
            if q == b and x < M:
                break
            x = down(x) if (q > b or x >= M) else up(x)
        assert np.rint(x * a) == b and (x < M or b == 0), (b, M)
        out[b] = x
    return out


def field_from_bins(bins, M, max_pos):
    """bins: [H][W] wanted bin per pixel (255 at max_pos) -> u (alternating sign), v = 0, identity"""
    bins = np.asarray(bins); assert bins[max_pos] == 255
    u = bin_values(M)[bins]; u[max_pos] = f32(M)
    u.ravel()[1::2] *= f32(-1.0)
    return np.ascontiguousarray(u, f32), np.zeros(bins.shape, f32), EYE.copy()


def bins_from_hist(hist, W, H, max_pos=None, seed=0):
    """a pixel layout with the wanted histogram: shuffled, one pixel of bin 255 at max_pos (default: somewhere in the middle)"""
    hist = np.asarray(hist); assert hist.sum() == W * H and hist[255] >= 1
    if max_pos is None:
        max_pos = (H // 2, W // 2 + 1)
    h = hist.copy(); h[255] -= 1
    rest = np.repeat(np.arange(256), h); np.random.default_rng(seed).shuffle(rest)
    flat = max_pos[0] * W + max_pos[1]
    return np.insert(rest, flat, 255).reshape(H, W), max_pos


def spikes(N, pairs):
    h = np.zeros(256, np.int64)
    for b, n in pairs:
        h[b] += n
    assert h.sum() == N and (h >= 0).all(), pairs
    return h


# ---------------------------------------------------------------------------------------------------------------- the family of histograms
class Family:
    pass


_families = {}


def family(N):
    """a fixed family of histograms summing to N with the reference's Otsu and Triangle values: first those with a pixel in bin 255 (each can be a field), then
    some without (in a frame of 64 pixels the one pixel in bin 255 decides Otsu's value, and a few rules cannot be reached with it)"""
    if N in _families:
        return _families[N]
    hs = []
    half = N // 2
    for a in (0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 17, 20, 40, 99, 100):                  # structured: the count rule sits on N / 2
        for b in (a + 1, a + 2, a + 5, a + 30, 200):
            if b >= 255:
                continue
            hs.append(spikes(N, [(a, half), (b, half - 1), (255, 1)]))
            hs.append(spikes(N, [(a, half - 1), (b, half), (255, 1)]))
            if half >= 3:
                hs.append(spikes(N, [(a, half - 1), (b, half - 1), (b + 3, 1), (255, 1)]))
                hs.append(spikes(N, [(a, half), (b, half - 2), (b + 1, 1), (255, 1)]))
    rng = np.random.default_rng(20240 + N)
    for k in range(2600):                                                                # a few occupied bins, mostly low ones, and a tail
        nb = int(rng.integers(2, 7))
        pool = np.arange(0, 14) if k % 3 else np.concatenate([np.arange(0, 24), np.arange(90, 112), [150, 200, 254]])
        bins = rng.choice(pool, min(nb, len(pool)), replace=False)
        if k % 5 == 0:                                                                   # contiguous run: Otsu has no flat stretch
            lo = int(rng.integers(0, 12)); bins = np.arange(lo, lo + nb)
        wts = rng.dirichlet(np.full(len(bins), 0.7))
        n255 = 1 if k % 4 else int(rng.integers(1, max(2, N // 8)))
        cnt = np.floor(wts * (N - n255)).astype(np.int64); cnt[int(np.argmax(cnt))] += (N - n255) - cnt.sum()
        hs.append(spikes(N, list(zip(bins.tolist(), cnt.tolist())) + [(255, n255)]))
    for k in range(600):                                                                 # a run of low bins around an almost empty bin 5 (Otsu 5 below Triangle 6)
        lo = int(rng.integers(1, 5)); bins = np.arange(lo, int(rng.integers(6, 12)) + 1)
        cnt = np.floor(rng.dirichlet(np.full(len(bins), 0.7)) * (N - 1)).astype(np.int64)
        cnt[5 - lo] = min(cnt[5 - lo], int(rng.integers(0, 2))); cnt[int(np.argmax(cnt))] += (N - 1) - cnt.sum()
        hs.append(spikes(N, list(zip(bins.tolist(), cnt.tolist())) + [(255, 1)]))
    hs2 = []
    for k in range(1500):                                                                # nothing in bin 255: these exist as blocks only, and are tried last
        nb = int(rng.integers(2, 8)); lo = int(rng.integers(0, 10))
        bins = np.arange(lo, lo + nb) if k % 2 else rng.choice(np.arange(0, 24), nb, replace=False)
        cnt = np.floor(rng.dirichlet(np.full(nb, 0.7)) * N).astype(np.int64); cnt[int(np.argmax(cnt))] += N - cnt.sum()
        hs2.append(spikes(N, list(zip(bins.tolist(), cnt.tolist()))))
    F = Family(); F.N = N
    F.hists = np.concatenate([np.unique(np.array(hs, np.int64), axis=0), np.unique(np.array(hs2, np.int64), axis=0)])
    F.otsu = R.otsu(F.hists, N)[0]
    F.tri = np.array([R.triangle(h) for h in F.hists])
    _families[N] = F
    return F


def exact_quotient(c, t):
    """M with float32(c) / M == t exactly (and M exactly c / t), or None"""
    if t <= 0:
        return None
    M = f32(c) / f32(t)
    return M if (f64(M) * f64(t) == f64(c) and f32(c) / M == f32(t)) else None


# ---------------------------------------------------------------------------------------------------------------- rule scenes as (hist, M) blocks
C17, C30, C100 = f32(1.7) * f32(255.0), f32(3.0) * f32(255.0), f32(10.0) * f32(255.0)


def _rec_is(want):
    return lambda r: all(k in r["rec"] and r["rec"][k] == v for k, v in want.items())


def _edge_rule(F, W, H, name, const, qname, which, on_eq, on_above, on_below, extra=lambda o, t: True, also=None):
    """a clamp comparison against the quotient `qname` = const / M: the first histogram of the family for which, with M = const / threshold exactly, the
    reference's record shows the quotient equal to the threshold (record on_eq) and, at the two neighbouring floats of M, one ulp above (on_above) and one ulp
    below it (on_below).  which(otsu, tri) -> the integer threshold the comparison looks at."""
    for k in range(len(F.hists)):
        o, t = F.otsu[k], F.tri[k]
        if not extra(o, t):
            continue
        thr = which(o, t); M0 = exact_quotient(const, thr)
        if M0 is None:
            continue
        trio = []
        for tag, M, q, want in (("eq", M0, f32(thr), on_eq), ("q_above", down(M0), up(thr), on_above), ("q_below", up(M0), down(thr), on_below)):
            want = dict(want); want[qname] = q
            if also:
                want.update(also)
            lo, hi, rec = R.clamp(F.hists[k], W, H, M, o, t)
            if not all(kk in rec and rec[kk] == v for kk, v in want.items()):
                break
            trio.append(Scene(f"{name}.{tag}", f"otsu {o:g}, triangle {t:g}, M {M!r}: " + ", ".join(f"{a} == {b!r}" for a, b in want.items()),
                              _rec_is(want), W, H, hist=F.hists[k].astype(np.int32), M=M))
        if len(trio) == 3:
            return trio
    raise AssertionError(f"no histogram of the family sits on {name} at {W} x {H}")


def _find(F, W, H, name, prop, Ms, pred):
    """the first (histogram, M) of the family x Ms whose reference record satisfies pred(rec, lo, hi, otsu, tri, hist)"""
    for k in range(len(F.hists)):
        for M in Ms:
            lo, hi, rec = R.clamp(F.hists[k], W, H, f32(M), F.otsu[k], F.tri[k])
            if pred(rec, lo, hi, F.otsu[k], F.tri[k], F.hists[k]):
                return Scene(name, prop, lambda r, p=pred: p(r["rec"], r["lo"], r["hi"], f64(r["otsu"]), f64(r["triangle"]), r["hist"]), W, H,
                             hist=F.hists[k].astype(np.int32), M=f32(M))
    raise AssertionError(f"no histogram of the family gives {name} at {W} x {H}")


_rule_cache = {}


def rule_blocks(W, H):
    """the clamp, count and branch scenes as (hist, M) blocks; a histogram with a pixel in bin 255 is a field as well"""
    if (W, H) in _rule_cache:
        return _rule_cache[(W, H)]
    F = family(W * H); N = W * H; out = []
    A = lambda o, t: o < t
    B = lambda o, t: o >= t
    T, Fa = True, False
    # branch A (otsu < triangle): thred1 = otsu against 1.7 * 255 / M and 3 * 255 / M, thred2 = triangle against max(3 * 255 / M, thred1 * 1.2f) and 10 * 255 / M
    out += _edge_rule(F, W, H, "A.lt17", C17, "q17", lambda o, t: o, {"A.lt17": Fa}, {"A.lt17": T}, {"A.lt17": Fa}, A, {"otsu<tri": T})
    out += _edge_rule(F, W, H, "A.gt30", C30, "q30", lambda o, t: o, {"A.lt17": Fa, "A.gt30": Fa}, {"A.gt30": Fa}, {"A.gt30": T}, A, {"otsu<tri": T})
    out += _edge_rule(F, W, H, "A.ltmax.arm1", C30, "q30", lambda o, t: t, {"A.arm2": Fa, "A.ltmax": Fa}, {"A.arm2": Fa, "A.ltmax": T}, {"A.arm2": Fa, "A.ltmax": Fa}, A, {"otsu<tri": T})
    out += _edge_rule(F, W, H, "A.ltmax.arm2_is_6", C30, "q30", lambda o, t: t, {"A.arm2": Fa, "A.ltmax": Fa, "A.arm": f32(6.0)}, {"A.arm2": Fa, "A.ltmax": T, "A.arm": f32(6.0)},
                      {"A.arm2": T, "A.ltmax": Fa, "A.arm": f32(6.0)}, lambda o, t: o == 5 and t == 6, {"otsu<tri": T, "A.count>half": Fa})
    out += _edge_rule(F, W, H, "A.gt100", C100, "q100", lambda o, t: t, {"A.ltmax": Fa, "A.gt100": Fa}, {"A.ltmax": Fa, "A.gt100": Fa}, {"A.ltmax": Fa, "A.gt100": T}, A, {"otsu<tri": T})
    # branch B (otsu >= triangle): the same with the roles swapped, and no count rule
    out += _edge_rule(F, W, H, "B.lt17", C17, "q17", lambda o, t: t, {"B.lt17": Fa}, {"B.lt17": T}, {"B.lt17": Fa}, B, {"otsu<tri": Fa})
    out += _edge_rule(F, W, H, "B.gt30", C30, "q30", lambda o, t: t, {"B.lt17": Fa, "B.gt30": Fa}, {"B.gt30": Fa}, {"B.gt30": T}, B, {"otsu<tri": Fa})
    out += _edge_rule(F, W, H, "B.ltmax.arm1", C30, "q30", lambda o, t: o, {"B.arm2": Fa, "B.ltmax": Fa}, {"B.arm2": Fa, "B.ltmax": T}, {"B.arm2": Fa, "B.ltmax": Fa}, B, {"otsu<tri": Fa})
    out += _edge_rule(F, W, H, "B.ltmax.arm2_is_6", C30, "q30", lambda o, t: o, {"B.arm2": Fa, "B.ltmax": Fa, "B.arm": f32(6.0)}, {"B.arm2": Fa, "B.ltmax": T, "B.arm": f32(6.0)},
                      {"B.arm2": T, "B.ltmax": Fa, "B.arm": f32(6.0)}, lambda o, t: o == 6 and t == 5, {"otsu<tri": Fa})
    out += _edge_rule(F, W, H, "B.gt100", C100, "q100", lambda o, t: o, {"B.ltmax": Fa, "B.gt100": Fa}, {"B.ltmax": Fa, "B.gt100": Fa}, {"B.ltmax": Fa, "B.gt100": T}, B, {"otsu<tri": Fa})
    Ms = [20.0, 30.0, 41.25, 63.75, 70.0, 80.0, 100.0, 127.5, 144.5, 200.0, 255.0, 400.0]
    # the second arm of the maximum alone decides (thred * 1.2f above 3 * 255 / M and above the other threshold)
    out.append(_find(F, W, H, "A.arm2_raises", "otsu < triangle, thred1 * 1.2f > 3 * 255 / M and > triangle: thred2 = thred1 * 1.2f", Ms,
                     lambda rec, lo, hi, o, t, h: rec.get("A.arm2") is True and rec.get("A.ltmax") is True and hi == rec["A.arm"]))
    out.append(_find(F, W, H, "B.arm2_raises", "otsu >= triangle, thred2 * 1.2f > 3 * 255 / M and > otsu: thred1 = thred2 * 1.2f", Ms,
                     lambda rec, lo, hi, o, t, h: rec.get("B.arm2") is True and rec.get("B.ltmax") is True and hi == rec["B.arm"]))
    # the count rule: pixels above the clamped thred1 exactly N / 2 (not taken) and N / 2 + 1 (taken); then a frame where the raised thred1 decides the next comparison
    out.append(_find(F, W, H, "A.count_is_half", "otsu < triangle, pixels above the clamped thred1 == N / 2: not raised", Ms,
                     lambda rec, lo, hi, o, t, h: rec.get("A.count") == N // 2 and N % 2 == 0 and rec["A.count>half"] is False and lo == rec["A.t1_before_count"]))
    out.append(_find(F, W, H, "A.count_is_half_plus_1", "otsu < triangle, pixels above the clamped thred1 == N / 2 + 1: raised by 0.2f * 255 / M", Ms,
                     lambda rec, lo, hi, o, t, h: rec.get("A.count") == N // 2 + 1 and rec["A.count>half"] is True and lo > rec["A.t1_before_count"]))
    out.append(_find(F, W, H, "A.count_raise_feeds_on", "count rule taken, and triangle < raised thred1 * 1.2f although triangle >= max(3 * 255 / M, unraised thred1 * 1.2f)", Ms,
                     lambda rec, lo, hi, o, t, h: rec.get("A.count>half") is True and rec["A.ltmax"] is True and rec["A.arm2"] is True and
                     f32(t) >= max(rec["q30"], rec["A.t1_before_count"] * f32(1.2))))
    # branch choice: the tie takes the else branch
    out.append(_find(F, W, H, "branch.tie", "otsu == triangle: the else branch", Ms, lambda rec, lo, hi, o, t, h: o == t and rec["otsu<tri"] is False))
    out.append(_find(F, W, H, "branch.otsu_above", "otsu > triangle", Ms, lambda rec, lo, hi, o, t, h: o > t and rec["otsu<tri"] is False))
    out.append(_find(F, W, H, "branch.otsu_below", "otsu < triangle", Ms, lambda rec, lo, hi, o, t, h: o < t and rec["otsu<tri"] is True))
    # masks: integer thresholds with pixels exactly on them and one above them
    out.append(_find(F, W, H, "mask.integer_thresholds", "lo and hi integers, pixels in bins lo, lo + 1, hi, hi + 1: q == thr is not set, q == thr + 1 is", [255.0, 127.5, 63.75, 510.0],
                     lambda rec, lo, hi, o, t, h: lo == np.floor(lo) and hi == np.floor(hi) and 0 < hi < 255 and lo < hi and h[int(lo)] > 0 and h[int(lo) + 1] > 0 and h[int(hi)] > 0 and h[int(hi) + 1] > 0))
    _rule_cache[(W, H)] = out
    return out


def _tri_is(left, right, max_ind, flipped, tri):
    return lambda r: (r["rec"]["tri_left"], r["rec"]["tri_right"], r["rec"]["tri_max_ind"], r["rec"]["tri_flipped"], float(r["triangle"])) == (left, right, max_ind, flipped, float(tri))


def shape_blocks(W, H):
    """Otsu's and Triangle's own edge cases as (hist, M) blocks.  Some have no pixel in bin 255, so they exist as blocks only."""
    N = W * H; out = []; M = f32(37.0)

    def blk(name, prop, holds, pairs, M=M):
        out.append(Scene(name, prop, holds, W, H, hist=spikes(N, pairs).astype(np.int32), M=f32(M)))
    for b in (0, 255, 97):
        blk(f"otsu.one_bin_{b}", f"everything in bin {b}: every bin is skipped, Otsu returns 0", lambda r: r["otsu"] == 0, [(b, N)])
        if b != 255:
            blk(f"otsu.one_bin_{b}_and_a_pixel", f"N - 1 pixels in bin {b}, one in bin 255", lambda r, b=b: r["hist"][b] == N - 1 and r["hist"][255] == 1, [(b, N - 1), (255, 1)])
    blk("otsu.one_bin_255_and_a_pixel", "N - 1 pixels in bin 255, one in bin 0", lambda r: r["hist"][255] == N - 1, [(0, 1), (255, N - 1)])
    for a, b in ((3, 200), (0, 255), (100, 101), (17, 23)):
        blk(f"otsu.two_equal_spikes_{a}_{b}", f"N / 2 pixels in each of the bins {a} and {b}: sigma is flat between them, rounding decides, first maximum wins",
            lambda r, a=a, b=b: a <= r["otsu"] < b, [(a, N // 2), (b, N - N // 2)])
    n4 = N // 4
    blk("otsu.symmetric", "a histogram symmetric about 127.5", lambda r: np.array_equal(r["hist"], r["hist"][::-1]), [(10, n4), (120, N // 2 - n4), (135, N // 2 - n4), (245, n4)])
    if N >= 64 * 8:
        sym = np.zeros(256, np.int64); k = N // 512; sym[:] = k; sym[127] += (N - 256 * k) // 2; sym[128] += (N - 256 * k) // 2
        out.append(Scene("otsu.symmetric_flat", "the same count in every bin, the remainder split over the two middle bins", lambda r: np.array_equal(r["hist"], r["hist"][::-1]), W, H,
                         hist=sym.astype(np.int32), M=M))
    # Triangle: left = 99, right = 161 after the widening, the peak in the middle (not flipped) and one bin to the left of it (flipped)
    big = N - 2
    blk("tri.peak_in_the_middle", "max_ind - left == right - max_ind: not flipped", lambda r: r["rec"]["tri_max_ind"] - r["rec"]["tri_left"] == r["rec"]["tri_right"] - r["rec"]["tri_max_ind"]
        and r["rec"]["tri_flipped"] is False, [(100, 1), (130, big), (160, 1)])
    blk("tri.peak_one_left_of_the_middle", "max_ind - left == right - max_ind - 2: flipped", lambda r: r["rec"]["tri_max_ind"] - r["rec"]["tri_left"] == r["rec"]["tri_right"] - r["rec"]["tri_max_ind"] - 2
        and r["rec"]["tri_flipped"] is True, [(100, 1), (129, big), (160, 1)])
    blk("tri.peak_one_right_of_the_middle", "max_ind - left == right - max_ind + 2: not flipped", lambda r: r["rec"]["tri_flipped"] is False and r["rec"]["tri_max_ind"] == 131, [(100, 1), (131, big), (160, 1)])
    e = (N - 2) // 2
    blk("tri.equal_peaks", "two equal peaks: the first is the maximum", lambda r: r["rec"]["tri_max_ind"] == 40, [(40, e), (180, e), (250, N - 2 * e)])
    blk("tri.ends_occupied", "bins 0 and 255 occupied: no widening of the bounds", lambda r: (r["rec"]["tri_left"], r["rec"]["tri_right"]) == (0, 255), [(0, 1), (60, N - 2), (255, 1)])
    blk("tri.peak_at_255", "the peak in bin 255", lambda r: r["rec"]["tri_max_ind"] == 255 and r["rec"]["tri_flipped"] is False, [(3, 1), (255, N - 1)])
    blk("tri.peak_at_0", "the peak in bin 0", lambda r: r["rec"]["tri_max_ind"] == 0 and r["rec"]["tri_flipped"] is True, [(0, N - 1), (255, 1)])
    # staircases: the counts lie on the line from (left, 0) to the peak, so a * i + b * h[i] takes the same positive value on every step and the first step wins
    steps = 6 if N >= 64 * 8 else 3; T = steps * (steps + 1) // 2; c = N // (T + steps) + 1; rest = N - c * T
    assert 0 <= rest < steps * c                                                         # the bin behind the peak stays below the peak
    for name, flip in (("tri.staircase_up", False), ("tri.staircase_down", True)):
        pairs = [(20 + s, s * c) for s in range(1, steps + 1)] + ([(20 + steps + 1, rest)] if rest else [])
        if flip:
            pairs = [(255 - b, n) for b, n in pairs]
        blk(name, "a staircase up to the peak: equal distances, the first step wins", lambda r, flip=flip: r["rec"]["tri_flipped"] is flip and r["triangle"] == (235 if flip else 20), pairs)
    return out


def hist_kinds(rng, n, N):
    """n histograms of the ten kinds test_thresholds_gpu.py draws (residual-like, two populations, one bin, two spikes, uniform, a pixel or two away from bin 0, peak
    at the right end, sparse, equal peaks, narrow band), rescaled to N pixels: the kinds that are a density are drawn with at most 65 536 samples and scaled to N
    (the remainder goes to the fullest bin), the others are counted out directly.  The 257th word holds the maximal residual."""
    out = np.zeros((n, 257), np.int32); ns = min(N, 1 << 16)
    for k in range(n):
        kind = k % 10; v = None; h = np.zeros(256, np.int64)
        if kind == 0:
            v = np.minimum(rng.gamma(1.5, rng.uniform(3, 40), ns), 255).astype(np.int64); v[0] = 255
        elif kind == 1:
            v = np.where(rng.random(ns) < rng.uniform(0.05, 0.6), rng.normal(rng.uniform(120, 230), 12, ns), rng.normal(rng.uniform(5, 60), 6, ns)).clip(0, 255).astype(np.int64)
        elif kind == 2:
            h[rng.integers(0, 256)] = N
        elif kind == 3:
            a, b = rng.integers(0, 256, 2); na = min(N - 1, max(1, int(rng.uniform(0.001, 0.999) * N))); h[a] += na; h[b] += N - na
        elif kind == 4:
            v = rng.integers(0, 256, ns)
        elif kind == 5:
            m = int(rng.integers(1, 3)); h[rng.integers(1, 256)] = m; h[0] = N - m
        elif kind == 6:
            v = (255 - np.minimum(rng.gamma(2.0, rng.uniform(2, 30), ns), 255)).astype(np.int64)
        elif kind == 7:
            bins = rng.choice(256, rng.integers(2, 7), replace=False); v = rng.choice(bins, ns)
        elif kind == 8:
            for j, b in enumerate(rng.choice(256, 3, replace=False)):                    # N // 3 + 1 pixels in the first bins, the rest in the last: equal peaks
                h[b] = min(N // 3 + 1, N - j * (N // 3 + 1))
        else:
            lo = rng.integers(0, 200); v = rng.integers(lo, lo + rng.integers(2, 56), ns)
        if v is not None:
            h = np.bincount(v, minlength=256).astype(np.int64) * N // ns; h[int(np.argmax(h))] += N - h.sum()
        assert h.sum() == N and (h >= 0).all()
        out[k, :256] = h
        out[k, 256] = np.float32(rng.uniform(0.3, 80.0)).view(np.int32)
    return out


def blocks(W, H):
    return rule_blocks(W, H) + shape_blocks(W, H)


# ---------------------------------------------------------------------------------------------------------------- field scenes
def _field(name, prop, holds, W, H, u, v, Hm):
    return Scene(name, prop, holds, W, H, u=np.ascontiguousarray(u, f32), v=np.ascontiguousarray(v, f32), Hm=np.asarray(Hm, f64).copy())


def rule_fields(W, H):
    """every block scene that has a pixel in bin 255, as a flow field with that histogram and maximum"""
    out = []
    for k, s in enumerate(blocks(W, H)):
        if s.hist[255] < 1:
            continue
        bins, pos = bins_from_hist(s.hist, W, H, seed=k)
        u, v, Hm = field_from_bins(bins, s.M, pos)
        out.append(_field(s.name, s.prop + "; the field has the block's histogram and maximum",
                          lambda r, s=s: np.array_equal(r["hist"], s.hist) and r["maxError"] == s.M and s.holds(r), W, H, u, v, Hm))
    return out


def rounding_fields(W, H):
    N = W * H; out = []; z = np.zeros((H, W), f32)
    # mag * a exactly on k + 0.5, one float below, one float above; a = 1 (M = 255) and a = 0.5f (M = 510, odd u)
    for M, scale in ((255.0, 1.0), (510.0, 2.0)):
        k = np.arange(N) % 254; tie = ((k + 0.5) * scale).astype(f32)
        assert np.array_equal(tie.astype(f64), (k + 0.5) * scale)
        kind = (np.arange(N) // 254 + np.arange(N)) % 3                                       # 0: the tie, 1: one float below, 2: one float above
        u = np.where(kind == 0, tie, np.where(kind == 1, np.nextafter(tie, f32(0)), np.nextafter(tie, f32(np.inf)))).astype(f32)
        want = np.where(kind == 0, k + (k % 2), np.where(kind == 1, k, k + 1))               # half to even; below -> k; above -> k + 1
        u[N - 1] = M; want[N - 1] = 255
        u[::3] *= f32(-1.0)
        out.append(_field(f"round.ties_M{int(M)}", f"M = {M}: mag * a on k + 0.5 for even and odd k rounds to even; one float below gives k, one above k + 1",
                          lambda r, want=want: np.array_equal(r["mag_u8"].ravel(), want),
                          W, H, u.reshape(H, W), z, EYE))
    # an a that is no power of two; a huge and a tiny maximum; no motion at all
    hist = np.zeros(256, np.int64); hist[:] = N // 256; hist[255] += 1; hist[0] += N - hist.sum()
    for M in (f32(3.0), f32(0.3)):
        bins, pos = bins_from_hist(hist, W, H, seed=3)
        u, v, Hm = field_from_bins(bins, M, pos)
        out.append(_field(f"round.M{float(M):.1f}", f"M = {M!r}: a = float32(255 / M) is no power of two; the wanted histogram comes out",
                          lambda r, M=M, hist=hist: r["maxError"] == M and np.array_equal(r["hist"], hist), W, H, u, v, Hm))
    one = spikes(N, [(0, N - 1), (255, 1)])
    u = z.copy(); u[H // 2, W // 2 + 1] = 3.0e6
    out.append(_field("max.3e6", "one residual of 3e6, everything else in bin 0", lambda r: r["maxError"] == f32(3.0e6) and np.array_equal(r["hist"], one), W, H, u, z, EYE))
    tiny = up(f32(2.0 ** -75)); small = f32(np.sqrt(f32(2.0 ** -149)))
    assert tiny * tiny == f32(2.0 ** -149) and f32(2.0 ** -75) * f32(2.0 ** -75) == 0
    u = z.copy(); u[H - 1, W // 3] = tiny
    out.append(_field("max.smallest", "the smallest magnitude a square can yield: sqrt of the smallest subnormal", lambda r: r["maxError"] == small and np.array_equal(r["hist"], one), W, H, u, z, EYE))
    out.append(_field("max.zero", "identity and zero flow: M = 0, thresholds inf, masks empty, all N pixels in bin 0",
                      lambda r: r["maxError"] == 0 and r["hist"][0] == N and np.isinf(r["lo"]) and np.isinf(r["hi"]) and not r["mask_low"].any() and not r["mask_high"].any(), W, H, z, z, EYE))
    return out


def location_fields(W, H):
    """the maximum in one pixel only: first, last, a row of the last partial group of four rows, a column of the second, half-filled block of 128 columns"""
    N = W * H; out = []
    hist = spikes(N, [(1, N - N // 3 - 1), (9, N // 3), (255, 1)])
    spots = {"first_pixel": (0, 0), "last_pixel": (H - 1, W - 1)}
    if H % 4:
        spots["last_partial_row_group"] = (H - 1, W // 2)
    if W % 128:
        spots["half_filled_column_block"] = (H // 2, W - 2)
    for k, (name, pos) in enumerate(spots.items()):
        bins, pos = bins_from_hist(hist, W, H, max_pos=pos, seed=10 + k)
        u, v, Hm = field_from_bins(bins, f32(12.5), pos)
        out.append(_field(f"max_at.{name}", f"the maximum 12.5 in pixel {pos} only",
                          lambda r, pos=pos: r["maxError"] == f32(12.5) and (r["mag"] == f32(12.5)).sum() == 1 and r["mag"][pos] == f32(12.5) and np.array_equal(r["hist"], hist), W, H, u, v, Hm))
    return out


def mask_fields(W, H):
    """single set pixels at x = 63, x = 64, the last bit of the last word and the first bit of a row: everything else in bin 0"""
    spots = [(0, 63), (H - 1, W - 1), (H // 2, 0)] + ([(0, 64)] if W > 64 else [])
    spots = sorted(set(spots))
    bins = np.zeros((H, W), np.int64)
    for p in spots:
        bins[p] = 255
    u, v, Hm = field_from_bins(bins, f32(40.0), spots[0])
    flat = sorted(p[0] * W + p[1] for p in spots)
    return [_field("mask.single_pixels", f"exactly the pixels {spots} are set in both masks",
                   lambda r: np.flatnonzero(r["mask_low"]).tolist() == flat and np.flatnonzero(r["mask_high"]).tolist() == flat and set(np.unique(r["mask_low"])) == {0, 128}, W, H, u, v, Hm)]


def homography_fields(W, H):
    """smooth flow under a pure translation by 0.1 and under a perspective homography: the FP64 -> FP32 cast and the division (no rule to sit on)"""
    rng = np.random.default_rng(77 * W + H)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    u = (0.8 * np.sin(xx / 7.0) + 0.05 * yy + rng.normal(0, 0.3, (H, W))).astype(f32); v = (0.5 * np.cos(yy / 5.0) - 0.02 * xx + rng.normal(0, 0.3, (H, W))).astype(f32)
    u[H // 3: H // 3 + max(1, H // 4), W // 4: W // 4 + W // 5] += 6.0
    tr = np.array([1.0, 0.0, 0.1, 0.0, 1.0, 0.1, 0.0, 0.0, 1.0])
    pe = np.array([1.0 + 1e-3, 2e-4, 0.3, -3e-4, 1.0 - 2e-3, -0.2, 1e-6, -2e-6, 1.0])
    ok = lambda r: r["maxError"] > 1 and (r["hist"] > 0).sum() > 20
    return [_field("H.translation_0.1", "a pure translation by 0.1 under smooth flow: many occupied bins", ok, W, H, u, v, tr),
            _field("H.perspective", "a perspective homography under smooth flow: many occupied bins", ok, W, H, u, v, pe)]


_field_cache = {}


def fields(W, H):
    if (W, H) not in _field_cache:
        _field_cache[(W, H)] = rule_fields(W, H) + rounding_fields(W, H) + location_fields(W, H) + mask_fields(W, H) + homography_fields(W, H)
    return _field_cache[(W, H)]


def few_fields(W, H):
    """a handful for the production size: no family search (one rule frame on the 1.7 arm, M = 144.5: a two-bin head), the rounding, extreme and homography scenes"""
    N = W * H
    hist = spikes(N, [(3, N - N // 4 - 1), (4, N // 8), (9, N // 4 - N // 8), (255, 1)])
    bins, pos = bins_from_hist(hist, W, H, max_pos=(H - 1, W - 1), seed=5)
    u, v, Hm = field_from_bins(bins, f32(144.5), pos)
    rule = _field("rule.M144.5", "M = 144.5: 1.7f * 255 / M == 3.0f; the wanted histogram comes out", lambda r: r["rec"]["q17"] == f32(3.0) and np.array_equal(r["hist"], hist), W, H, u, v, Hm)
    return [rule] + rounding_fields(W, H) + homography_fields(W, H)
