"""Plain numpy statements of the GPU front of CalOccluded and of the depth normalisation, one operation at a time, FP32 where the reference is FP32
(oracle/dynadetect.hpp:245-260 and 365-367; reference DynaDetect.cc:429-482, 765-768).  TEST INFRASTRUCTURE ONLY.

    median5     medianBlur(5): the 13th of the 25 replicated-border neighbours, by sorting
    edge_rule   the 5 x 5 max-difference edge and the valid-area mask, with the quantities the rules compare (for the tie checks)
    opening     MORPH_OPEN with the 4 x 4 ellipse: erode, then dilate (the oracle's cv::erode / cv::dilate)
    depth_norm  u16 * (float)((1 / max) * 255), cvRound (round half to even), saturate to 8 bits
    front       all of it for one frame
"""
import numpy as np

import oracle_lib as O

F = np.float32


def median5(d):
    d = np.asarray(d); h, w = d.shape
    p = np.pad(d, 2, mode="edge")
    nb = np.stack([p[i:i + h, j:j + w] for i in range(5) for j in range(5)])
    return np.sort(nb, axis=0)[12]


def edge_rule(filt, depth_scale):
    """-> dict(edge, total_area: u8 images with the 3-px frame 0; depth_max; val_max, depth1, quotient: FP32 arrays of the inner pixels;
    half_margin: the values (depth1 - nb) - depth_max * 0.5f that lie within one unit of the skip rule's threshold)"""
    f = np.asarray(filt).astype(F); h, w = f.shape
    depth_max = F(f.max()); half = F(depth_max * F(0.5)); ds = F(depth_scale)
    d1 = f[3:h - 3, 3:w - 3]
    quotient = d1 / ds                                        # FP32 IEEE division
    total = (d1 > F(0)) & (quotient < F(6))
    val_max = np.zeros_like(d1); margins = []
    for i in range(-2, 3):
        for j in range(-2, 3):
            nb = f[3 + i:h - 3 + i, 3 + j:w - 3 + j]
            diff = d1 - nb                                    # integers below 2^17: exact
            skip = diff > half
            val_max = np.where(skip, val_max, np.maximum(val_max, np.abs(diff)))
            m = diff.astype(np.float64) - float(half); margins.append(np.unique(m[np.abs(m) <= 1.0]))
    e = (val_max > d1 * F(0.03)) & (val_max > F(400))
    edge = np.zeros((h, w), np.uint8); area = np.zeros((h, w), np.uint8)
    edge[3:h - 3, 3:w - 3] = e * np.uint8(255); area[3:h - 3, 3:w - 3] = total * np.uint8(255)
    return dict(edge=edge, total_area=area, depth_max=int(depth_max), val_max=val_max, depth1=d1, quotient=quotient,
                half_margin=np.unique(np.concatenate(margins)) if margins else np.zeros(0))


def opening(edge):
    return O.morph(O.morph(np.ascontiguousarray(edge), 4, "erode"), 4, "dilate")


def depth_norm_products(d):
    """the FP32 products the rounding sees (None for an all-zero frame: 1 / 0)"""
    d = np.asarray(d); dmax = int(d.max())
    if dmax == 0:
        return None
    a = F((1.0 / float(dmax)) * 255)
    return d.astype(F) * a


def depth_norm(d):
    p = depth_norm_products(d)
    if p is None:                                             # 0 * inf: the conversion of the NaN saturates to 0 on both sides
        return np.zeros(np.asarray(d).shape, np.uint8)
    return np.clip(np.rint(p), 0, 255).astype(np.uint8)       # np.rint: round half to even, as cvRound


def front(d, depth_scale):
    d = np.asarray(d, np.uint16)
    filt = median5(d); r = edge_rule(filt, depth_scale)
    return dict(filt=filt, max_filt=int(filt.max()), max_raw=int(d.max()), edge_pre=r["edge"], edge=opening(r["edge"]), total_area=r["total_area"],
                depth_n=depth_norm(d), rule=r)


STAGES = ["total_area", "kmeans_label", "centers", "grad_edge", "plane_contours", "occ2", "occ1"]


def oracle_stages(bgr, depth, K, frames=(2, 3)):
    """the oracle's DynaDetect primed with frames 1 and 0, then run over `frames`: per frame the stage outputs of test_detect_sequence, the piece count and the outputs"""
    ref = O.DynaDetect(bgr[1], bgr[0], *K); out = []
    for t in frames:
        rd, rl = ref.detect(bgr[t], depth[t]); r = ref.debug()
        o = {k: r[k].copy() for k in STAGES}; o.update(pieces=int(r["info"][2]), dyna=rd, label=rl, dilate15=O.dilate15(rd)); out.append(o)
    return out
