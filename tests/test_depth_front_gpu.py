"""GPU: the front of CalOccluded (k_median5_u16, k_max_u16, k_grad_edge, k_morph_e4) and the depth normalisation (k_depth_norm) through the production launchers
(sind_debug_depth_front) against the plain numpy references of depth_ref.py, on the crafted frames of depth_scene.py: content that sits on every threshold of the
rules, salt and pepper on every border, maxima at the first and the last pixel, and batches whose frames differ (a bright, an all-zero and a dim one), at sizes
down to 71 x 13 -- no multiple of the rows a thread walks nor of the eight samples of a 16-byte load.  Everything is an integer or 8 bits wide: equality.
test_depth_scene_cpu.py proves the references against the oracle and that the tie scenes hold their ties."""
import functools

import numpy as np
import pytest

import depth_ref as R
import depth_scene as S

pytestmark = pytest.mark.gpu
KEYS = ["filt", "edge_pre", "edge", "total_area", "depth_n"]


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    return S.front_frames(w, h)


@functools.lru_cache(maxsize=None)
def _ref(w, h, name, ds):
    return R.front(_frames(w, h)[name][0], ds)


def _compare(w, h, names, ds):
    from sindslam_amd.dyna import depth_front
    d = np.stack([_frames(w, h)[n][0] for n in names])
    g = depth_front(d, ds)
    for k, n in enumerate(names):
        r = _ref(w, h, n, ds); what = (w, h, names, ds, n)
        assert int(g["max_filt"][k]) == r["max_filt"] and int(g["max_raw"][k]) == r["max_raw"], (what, g["max_filt"], g["max_raw"], r["max_filt"], r["max_raw"])
        for key in KEYS:
            assert np.array_equal(g[key][k], r[key]), (what, key, int((g[key][k] != r[key]).sum()))


@pytest.mark.parametrize("w,h", S.FRONT_SIZES)
def test_single_frame_forms(w, h):
    """n == 1: the launches of the drop-in path (DynaTail::cal_occluded_p1, seg_and_merge)"""
    for name, (_, ds) in _frames(w, h).items():
        _compare(w, h, (name,), ds)
    # the tie scenes are worth nothing if the reference's edge is empty or full there
    assert 0 < (_ref(w, h, "ties_400", 5000.0)["edge_pre"] > 0).sum() and 0 < (_ref(w, h, "half_even", 5000.0)["edge"] > 0).sum() < w * h


@pytest.mark.parametrize("w,h", S.FRONT_SIZES)
def test_batched_forms_with_frames_that_differ(w, h):
    """n == 3: the launches of OccBatch::run, per-frame maxima slots; the all-zero frame of a batch reports the maximum 0 (its slot is cleared, not written) and a
    dim frame its own maximum, not the bright neighbour's"""
    for names, ds in S.front_batches(w, h):
        _compare(w, h, names, ds)
        _compare(w, h, names[::-1], ds)


def test_bad_arguments_are_refused():
    import ctypes as C
    from sindslam_amd._lib import lib, ptr
    d = np.zeros((1, 7, 7), np.uint16); o8 = np.zeros((1, 7, 7), np.uint8); m = np.zeros(2, np.uint32)
    f = lib().sind_debug_depth_front
    assert f(ptr(d), 1, 6, 7, C.c_float(5000), 0, ptr(d.copy()), ptr(m), ptr(o8), ptr(o8), ptr(o8), ptr(o8)) == -1
    assert f(ptr(d), 0, 7, 7, C.c_float(5000), 0, ptr(d.copy()), ptr(m), ptr(o8), ptr(o8), ptr(o8), ptr(o8)) == -1
    assert f(ptr(d), 1, 7, 7, C.c_float(0), 0, ptr(d.copy()), ptr(m), ptr(o8), ptr(o8), ptr(o8), ptr(o8)) == -1
    assert f(None, 1, 7, 7, C.c_float(5000), 0, ptr(d.copy()), ptr(m), ptr(o8), ptr(o8), ptr(o8), ptr(o8)) == -1
    from sindslam_amd.dyna import depth_front
    g = depth_front(np.full((7, 7), 9, np.uint16), 5000.0)                    # the smallest frame: one inner pixel
    assert g["max_filt"][0] == 9 and g["total_area"][0, 3, 3] == 255 and g["total_area"].sum() == 255 and not g["edge"].any() and (g["depth_n"] == 255).all()
