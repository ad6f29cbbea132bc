"""CPU: the inputs of tests/orb_scene.py do what they claim, on the oracle alone -- every geometry is inside the oracle's domain and
fills the levels it should, every content generator drives the branch it is named for, and the mask builder lands exactly on either
side of the extractor's 250-keypoint fallback.  (Counts in comments are the oracle's, measured when the tests were written.)"""
import numpy as np
import pytest

import oracle_lib as O
import orb_scene as S


@pytest.mark.parametrize("w,h,sf,nl", S.GEOMETRY)
def test_geometry_cases_run_in_the_oracle(w, h, sf, nl):
    assert S.oracle_can_take(w, h, sf, nl)
    ref = O.ORBextractor(S.NFEATURES, sf, nl, 15, 5)
    k, d = ref.extract(S.tex(w, h, w + h))
    assert len(k) >= 30 and d.shape == (len(k), 32)                                  # 33 (64 x 64) ... 1515 (515 x 389)
    sizes = [ref.level_size(lv) for lv in range(nl)]
    assert sizes == S.level_sizes(w, h, sf, nl)
    for lv, (lw, lh) in enumerate(sizes):
        assert (len(ref.fast_keypoints(lv)) > 0) == S.holds_cell(lw, lh), (lv, lw, lh)


def test_geometry_table_holds_the_edges_it_names():
    assert S.level_sizes(223, 223, 1.2, 8)[-1] == (62, 62) and S.holds_cell(62, 62) and not S.holds_cell(61, 62)
    assert S.level_sizes(150, 120, 1.2, 8)[4:] == [(72, 58), (60, 48), (50, 40), (42, 33)]
    assert [S.holds_cell(*s) for s in S.level_sizes(150, 120, 1.2, 8)] == [True] * 4 + [False] * 4
    assert np.round(np.float32(1000 - 32) / np.float32(260 - 32)) == 4                # four initial octree nodes
    # sizes the oracle must not be given: a 32-px level (96 x 66, 6 levels) and a level less than half as wide as tall (360 x 800)
    assert not S.oracle_can_take(96, 66, 1.2, 6) and not S.oracle_can_take(360, 800, 1.2, 8) and not S.oracle_can_take(92, 151, 1.2, 2)
    # the small size the handle re-use test shrinks to: 8 levels from 91 down to 25 px, none of them 32
    assert S.level_sizes(91, 91, 1.2, 8)[-1] == (25, 25) and S.oracle_can_take(91, 91, 1.2, 8)


def _fast_and_final(img, ini, mn):
    ref = O.ORBextractor(S.NFEATURES, 1.2, 8, ini, mn)
    k, _ = ref.extract(img)
    f = np.concatenate([ref.fast_keypoints(lv) for lv in range(8)])
    return np.stack([f["x"], f["y"], f["response"], f["octave"]], 1), k


@pytest.mark.parametrize("name", ["dots", "mixed_contrast"])
def test_both_fast_passes_decide_cells(name):
    """the (20, 7) list differs from (20, 20), so the retry decided some cells, and from (7, 7), so the first pass decided others"""
    img = S.CONTENT[name](320, 240, 1)
    both, _ = _fast_and_final(img, 20, 7); first, _ = _fast_and_final(img, 20, 20); retry, _ = _fast_and_final(img, 7, 7)
    assert len(first) < len(both) < len(retry)            # dots 146 / 149 / 180, mixed_contrast 3785 / 3918 / 4678
    assert not np.array_equal(both, first) and not np.array_equal(both, retry)


def test_low_contrast_lives_on_the_second_pass():
    img = S.low_contrast(320, 240, 1)
    assert len(_fast_and_final(img, 20, 20)[1]) == 0
    assert len(_fast_and_final(img, 20, 7)[1]) > 100                                  # 206


def test_binary_blocks_saturate_scores_and_pin_cardinal_angles():
    _, k = _fast_and_final(S.binary_blocks(320, 240), 20, 7)
    assert np.isin(k["angle"], [0.0, 90.0, 180.0, 270.0]).sum() >= 100                # 328
    assert k["response"].max() == 254


def test_mask_builder_lands_on_both_sides_of_the_fallback():
    img = S.tex(320, 240, 5)
    ref = O.ORBextractor(S.NFEATURES, 1.2, 8, 15, 5)
    k0, _ = ref.extract(img)
    assert len(k0) == 1507
    sel = [ref.selected(lv) for lv in range(8)]
    m249, n249 = S.mask_leaving(sel, 1.2, 249, img.shape); m250, n250 = S.mask_leaving(sel, 1.2, 250, img.shape)
    assert n249 == 249 and n250 == 250
    assert len(ref.extract(img, m249)[0]) == 1507         # 249 survivors: below the bar, every keypoint comes back
    assert len(ref.extract(img, m250)[0]) == 250          # 250 survivors: the erasure stands
