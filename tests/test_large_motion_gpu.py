"""GPU: the large-motion decision of the dense flow -- k_mag_max, k_mag_hist with blockIdx.y = image and the host rule DynaFront::dense_flow calls
(sind_debug_large_motion: the production launch_mag_stats with batch B, no DeepFlow, no sign flip) -- against the numpy restatement of the reference
(motion_ref.decide) on fields that sit ON the rule: flags, histograms, maxima, endFlow and endFlow2 are equal.  What the cases pin, and that the reference alone
separates both members of every pair, is asserted on the CPU (test_large_motion_cpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import motion_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cases(fw, fh, W, H):
    cs = R.cases(fw, fh, W, H)
    return cs, {n: R.decide(c["u"], c["v"], W, H) for n, c in cs.items()}


def _gpu(u, v, W, H):
    from sindslam_amd._lib import check, lib, ptr
    B, fh, fw = u.shape
    flags = np.full(B, -1, np.int32); hist = np.full((B, 256), -1, np.int32); mx = np.full(B, -1, np.float32); end = np.full((B, 2), -7, np.int32)
    check(lib().sind_debug_large_motion(ptr(u), ptr(v), B, fw, fh, W, H, 0, ptr(flags), ptr(hist), ptr(mx), ptr(end)), "sind_debug_large_motion")
    return flags, hist, mx, end


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("fw,fh,W,H", R.SIZES)
def test_decision_equals_the_reference(fw, fh, W, H, B):
    cs, ref = _cases(fw, fh, W, H)
    for names in R.batches(list(cs), B):
        u = np.ascontiguousarray(np.stack([cs[n]["u"] for n in names])); v = np.ascontiguousarray(np.stack([cs[n]["v"] for n in names]))
        flags, hist, mx, end = _gpu(u, v, W, H)
        for b, n in enumerate(names):
            r = ref[n]; what = (names, b, n)
            assert mx[b].view(np.uint32) == np.float32(r["max"]).view(np.uint32), (what, float(mx[b]), float(r["max"]))
            assert np.array_equal(hist[b], r["hist"]), (what, np.flatnonzero(hist[b] != r["hist"])[:8], hist[b][hist[b] != r["hist"]][:8], r["hist"][hist[b] != r["hist"]][:8])
            assert (int(end[b, 0]), int(end[b, 1])) == (r["endFlow"], r["endFlow2"]), (what, end[b].tolist(), r["endFlow"], r["endFlow2"])
            assert int(flags[b]) == r["flag"], what


def test_bad_arguments_are_refused():
    from sindslam_amd._lib import lib, ptr
    z = np.zeros((1, 4, 4), np.float32); f = np.zeros(1, np.int32)
    assert lib().sind_debug_large_motion(None, ptr(z), 1, 4, 4, 8, 8, 0, ptr(f), None, None, None) == -1
    assert lib().sind_debug_large_motion(ptr(z), ptr(z), 0, 4, 4, 8, 8, 0, ptr(f), None, None, None) == -1
    assert lib().sind_debug_large_motion(ptr(z), ptr(z), 1, 9, 4, 8, 8, 0, ptr(f), None, None, None) == -1          # the grid cannot be larger than the frame
    assert lib().sind_debug_large_motion(ptr(z), ptr(z), 1, 4, 4, 8, 8, 0, ptr(f), None, None, None) == 0 and f[0] == 1
