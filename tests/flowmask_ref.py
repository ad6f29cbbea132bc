"""The flow-mask stage (DynaDetect.cc:1252-1367: homography residual, u8 normalisation, 256-bin histogram, cv::threshold's Otsu and Triangle values, the
clamps, the two masks) restated in plain numpy, one IEEE operation per statement.  numpy's float32 / float64 scalars and arrays are IEEE binary32 / binary64
and round every operation once, so nothing here can contract into a fused multiply-add.  No kernel and no oracle code is used: tests compare both with this.

Out of scope: non-finite flow or homography, and a denominator that crosses zero inside the image."""
import numpy as np

f32 = np.float32
f64 = np.float64
FLT_EPSILON = f64(f32(1.1920928955078125e-7))


def residual(u, v, H):
    """-> (mag float32 [h][w], max float32): den, fx2, fy2 in float64 from converted integer col / row, cast to float32; the rest in float32"""
    u = np.asarray(u, f32); v = np.asarray(v, f32); h, w = u.shape
    H = np.asarray(H, f64).reshape(9)
    col = np.arange(w, dtype=np.int32).astype(f64)[None, :]; row = np.arange(h, dtype=np.int32).astype(f64)[:, None]
    with np.errstate(all="ignore"):
        t = H[6] * col; t2 = H[7] * row; t = t + t2; den = t + H[8]
        nx = H[0] * col; t2 = H[1] * row; nx = nx + t2; nx = nx + H[2]; nx = nx / den; fx2 = col - nx
        ny = H[3] * col; t2 = H[4] * row; ny = ny + t2; ny = ny + H[5]; ny = ny / den; fy2 = row - ny
        fx2 = fx2.astype(f32); fy2 = fy2.astype(f32)
        dx = u - fx2; dy = v - fy2
        a = dx * dx; b = dy * dy; s = a + b
        mag = np.sqrt(s)
    assert mag.dtype == f32 and s.dtype == f32
    m = f32(0.0)
    mm = mag.max()
    if mm > m:                                            # std::max(0.0f, ...) over the image: the largest value, or 0.0f
        m = mm
    return mag, m


def normalise(mag, m):
    """-> (q uint8 [h][w], hist int32 [256]): a = float32(255.0 / float64(max)); q = clamp(rint_half_even(mag * a), 0, 255); a NaN product (0 * inf when the
    maximum is 0) converts to the integer indefinite value, which is negative: bin 0"""
    with np.errstate(all="ignore"):
        a = f32(f64(255.0) / f64(m))
        x = mag * a
        assert x.dtype == f32
        r = np.rint(x)                                    # round half to even
    r = np.where(np.isnan(r), f32(-1.0), r)
    q = np.clip(r, 0, 255).astype(np.uint8)
    return q, np.bincount(q.ravel(), minlength=256).astype(np.int32)


def otsu(hists, N):
    """getThreshVal_Otsu_8u for K histograms at once ([K][256]; every statement below is one float64 operation on K lanes)
    -> (threshold float64 [K], mu1 chain float64 [K][256])"""
    hists = np.atleast_2d(np.asarray(hists)); K = hists.shape[0]
    hd = hists.astype(f64)
    scale = f64(1.0) / f64(N)
    mu = np.zeros(K, f64)
    for i in range(256):
        t = f64(i) * hd[:, i]; mu = mu + t
    mu = mu * scale
    mu1 = np.zeros(K, f64); q1 = np.zeros(K, f64); max_sigma = np.zeros(K, f64); max_val = np.zeros(K, f64)
    chain = np.zeros((K, 256), f64)
    one = f64(1.0); hi = one - FLT_EPSILON
    with np.errstate(all="ignore"):
        for i in range(256):
            p = hd[:, i] * scale
            mu1 = mu1 * q1
            q1 = q1 + p
            q2 = one - q1
            skip = (np.minimum(q1, q2) < FLT_EPSILON) | (np.maximum(q1, q2) > hi)
            t = f64(i) * p; t = mu1 + t; t = t / q1
            mu1 = np.where(skip, mu1, t)
            chain[:, i] = mu1
            t = q1 * mu1; t = mu - t; mu2 = t / q2
            d = mu1 - mu2
            s = q1 * q2; s = s * d; sigma = s * d
            better = ~skip & (sigma > max_sigma)          # strict: the first maximum wins
            max_sigma = np.where(better, sigma, max_sigma); max_val = np.where(better, f64(i), max_val)
    return max_val, chain


def triangle(hist, record=None):
    """getThreshVal_Triangle_8u (imgproc/thresh.cpp) -> threshold (float)"""
    h = [int(x) for x in hist]
    left = right = max_ind = mx = 0; flipped = False
    for i in range(256):
        if h[i] > 0:
            left = i; break
    if left > 0:
        left -= 1
    for i in range(255, 0, -1):
        if h[i] > 0:
            right = i; break
    if right < 255:
        right += 1
    for i in range(256):
        if h[i] > mx:
            mx = h[i]; max_ind = i
    if record is not None:
        record.update(tri_left=left, tri_right=right, tri_max_ind=max_ind)
    if max_ind - left < right - max_ind:
        flipped = True
        h = h[::-1]
        left = 255 - right; max_ind = 255 - max_ind
    thresh = float(left); a = float(mx); b = float(left - max_ind); dist = 0.0
    for i in range(left + 1, max_ind + 1):
        ta = a * float(i); tb = b * float(h[i]); t = ta + tb    # Python floats are binary64
        if t > dist:
            dist = t; thresh = float(i)
    thresh -= 1.0
    if flipped:
        thresh = 255.0 - thresh
    if record is not None:
        record.update(tri_flipped=flipped)
    return thresh


def _count_gt(hist, t):
    return int(sum(int(hist[b]) for b in range(256) if f64(b) > f64(t)))


def clamp(hist, W, H, m, otsu_v, tri_v):
    """DynaDetect.cc:1309-1367 in float32 -> (lo, hi, record).  record: every comparison that was evaluated (name -> bool), the quotients and the count"""
    m = f32(m)
    rec = {}
    with np.errstate(all="ignore"):
        c17 = f32(1.7) * f32(255.0); c30 = f32(3.0) * f32(255.0); c100 = f32(10.0) * f32(255.0); c02 = f32(0.2) * f32(255.0)
        q17 = c17 / m; q30 = c30 / m; q100 = c100 / m; q02 = c02 / m
        t1 = f32(otsu_v); t2 = f32(tri_v)
        rec.update(q17=q17, q30=q30, q100=q100)

        def smax(a, b):                                   # std::max(a, b)
            return b if a < b else a
        rec["otsu<tri"] = bool(t1 < t2)
        if t1 < t2:
            rec["A.lt17"] = bool(t1 < q17)
            if t1 < q17:
                t1 = q17
            else:
                rec["A.gt30"] = bool(t1 > q30)
                if t1 > q30:
                    t1 = q30
            cnt = _count_gt(hist, t1)
            half = f64(0.5) * f64(W); half = half * f64(H)
            rec["A.count"] = cnt; rec["A.count>half"] = bool(f64(cnt) > half); rec["A.t1_before_count"] = t1
            if f64(cnt) > half:
                t1 = t1 + q02
            arm = t1 * f32(1.2)
            rec["A.arm2"] = bool(q30 < arm); rec["A.arm"] = arm
            mx = smax(q30, arm)
            rec["A.ltmax"] = bool(t2 < mx)
            if t2 < mx:
                t2 = mx
            else:
                rec["A.gt100"] = bool(t2 > q100)
                if t2 > q100:
                    t2 = q100
            lo, hi = t1, t2
        else:
            rec["B.lt17"] = bool(t2 < q17)
            if t2 < q17:
                t2 = q17
            else:
                rec["B.gt30"] = bool(t2 > q30)
                if t2 > q30:
                    t2 = q30
            arm = t2 * f32(1.2)
            rec["B.arm2"] = bool(q30 < arm); rec["B.arm"] = arm
            mx = smax(q30, arm)
            rec["B.ltmax"] = bool(t1 < mx)
            if t1 < mx:
                t1 = mx
            else:
                rec["B.gt100"] = bool(t1 > q100)
                if t1 > q100:
                    t1 = q100
            lo, hi = t2, t1
    assert type(lo) is f32 and type(hi) is f32
    return lo, hi, rec


COMPARISONS = ["otsu<tri", "A.lt17", "A.gt30", "A.count>half", "A.arm2", "A.ltmax", "A.gt100", "B.lt17", "B.gt30", "B.arm2", "B.ltmax", "B.gt100"]


def thresholds(hist, W, H, m, otsu_v=None):
    """(hist, max) -> dict(otsu, triangle, lo, hi, rec); otsu_v may be passed when it was computed in a batch"""
    rec = {}
    if otsu_v is None:
        otsu_v = otsu(hist, W * H)[0][0]
    tri_v = triangle(hist, rec)
    lo, hi, r = clamp(hist, W, H, m, otsu_v, tri_v); rec.update(r)
    return dict(otsu=f32(otsu_v), triangle=f32(tri_v), lo=lo, hi=hi, rec=rec)


def masks(q, lo, hi):
    ql = q.astype(f64)
    return np.where(ql > f64(lo), 128, 0).astype(np.uint8), np.where(ql > f64(hi), 255, 0).astype(np.uint8)


def stage(u, v, H):
    """the whole stage on one frame"""
    h, w = np.asarray(u).shape
    mag, m = residual(u, v, H)
    q, hist = normalise(mag, m)
    t = thresholds(hist, w, h, m)
    ml, mh = masks(q, t["lo"], t["hi"])
    return dict(mag=mag, maxError=m, mag_u8=q, hist=hist, otsu=t["otsu"], triangle=t["triangle"], lo=t["lo"], hi=t["hi"], mask_low=ml, mask_high=mh, rec=t["rec"])
