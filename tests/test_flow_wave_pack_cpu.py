"""CPU: how k_sor_wave cuts its column strips over groups of images laid side by side (sind_flow_wave_pack_layout, host arithmetic only)."""
import ctypes as C

import numpy as np
import pytest

from sindslam_amd._lib import lib

BATCHES = (1, 2, 3, 19, 80, 171, 512)
HALO, LANE_COLS = 10, 128


def packed(w, h, B, group, items=0, bands=0):
    out = (C.c_int * 6)()
    assert lib().sind_flow_wave_pack_layout(w, h, B, items, bands, group, out) == 0
    return tuple(out)


def unpacked(w, h, B, items=0, bands=0):
    out = (C.c_int * 4)()
    assert lib().sind_flow_wave_layout(w, h, B, items, bands, out) == 0
    return tuple(out)


def check_cover(w, B, G, Pw, strips, IW):
    """the strips of a group of G images (and of a short last group) partition the virtual row; a strip's kept columns and the halo of each cut side fit a wave"""
    assert Pw % 2 == 0 and Pw >= w + 1 and IW % 2 == 0 and 1 <= G <= min(B, 32), (w, B, G, Pw, IW)
    for present in {G, B % G or G}:
        vw = (present - 1) * Pw + w
        if present == G:
            assert (strips - 1) * IW < vw <= strips * IW, (w, B, G, strips, IW)          # every column in exactly one strip, no strip empty
        kept = np.zeros(vw, np.int32)                                                     # times each column of the virtual row is kept
        for s in range(strips):
            ix0, ix1 = s * IW, min(s * IW + IW, vw)
            if ix0 >= vw:                                                                 # (beyond a short last group)
                continue
            ex0 = max(ix0 - HALO, 0)
            assert ex0 % 2 == 0 and ix1 + (HALO if ix1 < vw else 0) <= ex0 + LANE_COLS, (w, B, G, s, IW)
            kept[ix0:ix1] += 1
        image_column = np.arange(vw) % Pw < w
        assert image_column.sum() == w * present and (kept[image_column] == 1).all(), (w, B, G, present)


def test_packed_strips_cover_every_image_column_once_and_fit_a_wave():
    """w = 1 .. 700 at every batch size: the automatic group and forced groups of 2, 3, 5 and 32"""
    for w in range(1, 701):
        for B in BATCHES:
            n1, iw1, nb1, bh1 = unpacked(w, 173, B)
            for group in (0, 2, 3, 5, 32):
                G, Pw, strips, IW, nb, bh = packed(w, 173, B, group)
                assert (nb, bh) == (nb1, bh1), (w, B, group)                             # the row bands are the one-image layout's
                assert G == (min(group, B) if group else G)
                check_cover(w, B, G, Pw, strips, IW)
                if group == 0:
                    assert -(-B // G) * strips <= B * n1, (w, B, G, strips, n1)           # never more waves than one image per wave row
                    if G == 1:
                        assert (strips, IW) == (n1, iw1)


def test_group_of_one_is_the_one_image_layout():
    for w in range(1, 701):
        for B in BATCHES:
            for h, items, bands in ((173, 0, 0), (40, 2048, 0), (288, 0, 3)):
                G, Pw, strips, IW, nb, bh = packed(w, h, B, 1, items, bands)
                assert G == 1 and (strips, IW, nb, bh) == unpacked(w, h, B, items, bands), (w, h, B)


def brute_force(w, B):
    """the smallest groups x strips per group over the group sizes 1 .. 32 (the smaller size at a tie), with the strip rule written out again"""
    def strips_of(W):
        if W <= LANE_COLS:
            return 1
        n = 2
        while ((-(-W // n) + 1) & ~1) + (HALO if n == 2 else 2 * HALO) > LANE_COLS:
            n += 1
        return n
    Pw = (w + 2) & ~1
    return min((-(-B // G) * strips_of((G - 1) * Pw + w), G) for G in range(1, min(B, 32) + 1))


def test_automatic_group_needs_the_fewest_strips():
    for w in range(1, 701, 7):
        for B in BATCHES:
            G, Pw, strips, IW, _, _ = packed(w, 173, B, 0)
            assert (-(-B // G) * strips, G) == brute_force(w, B), (w, B)


@pytest.mark.parametrize("w,h,now,best", [(384, 288, 684, 612), (330, 247, 684, 531), (256, 191, 513, 414), (243, 181, 513, 387), (162, 120, 342, 261), (132, 98, 342, 215)])
def test_strips_per_launch_of_171_images(w, h, now, best):
    n1 = unpacked(w, h, 171)[0]
    G, _, strips, _, _, _ = packed(w, h, 171, 0)
    assert (171 * n1, -(-171 // G) * strips) == (now, best), (G, strips)


def test_large_planes_and_bad_arguments():
    """a group's planes stay below 2^31 bytes (a lane's offset within its group is 32 bits): 5000 x 4000 floats leave room for 26 images, 30000 x 10000 for one"""
    assert packed(5000, 4000, 64, 32)[0] == 26 and packed(30000, 10000, 64, 0)[0] == 1 and packed(30000, 10000, 64, 8)[0] == 1
    out = (C.c_int * 6)()
    f = lib().sind_flow_wave_pack_layout
    assert f(0, 10, 1, 0, 0, 0, out) == -1 and f(10, 0, 1, 0, 0, 0, out) == -1 and f(10, 10, 0, 0, 0, 0, out) == -1 and f(10, 10, 1, 0, 0, -1, out) == -1
    assert f(10, 10, 1, 0, 0, 0, None) == -1 and lib().sind_flow_set_wave_pack(None, 0) == -1
