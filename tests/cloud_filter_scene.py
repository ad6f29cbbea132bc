"""Scenes of the statistical outlier filter's tests (tests/test_cloud_filter_cpu.py, tests/test_cloud_filter_gpu.py) and the comparison both files use.
A scene is a function of mean_k that returns one cloud of POINT_DTYPE; the colours are random so that a permuted output shows."""
import functools

import numpy as np

import cloud_filter_ref as R
from sindslam_amd.cloud import MAX_MEAN_K, POINT_DTYPE

MEAN_KS = (1, 50, 100, MAX_MEAN_K)


def cloud(xyz, seed=7):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3); p = np.zeros(len(xyz), POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    c = np.random.default_rng(seed).integers(0, 256, (len(xyz), 4)).astype(np.uint8); p["b"], p["g"], p["r"], p["a"] = c.T
    return p


def random_far(mean_k=None):
    """4 000 points in the unit cube, every 37th NaN (some +-inf), a cluster of 60 points 1 000 units away (smaller than mean_k: its neighbours come from the main
    cloud) and one lone point at -500"""
    rng = np.random.default_rng(0); xyz = rng.random((4061, 3)).astype(np.float32)
    xyz[4000:4060] = 1000 + rng.random((60, 3)) * 0.1; xyz[4060] = -500
    xyz[::37] = np.nan; xyz[74, 1] = np.inf; xyz[111, 2] = -np.inf; xyz[148] = (0.5, np.nan, 0.5)
    return cloud(xyz)


def lattice(mean_k=None):
    g = np.arange(12, dtype=np.float32) * np.float32(0.125)
    return cloud(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1))


def coincident(mean_k=None):
    return cloud(np.tile(np.float32([0.25, -1.5, 3.0]), (150, 1)))


def exactly_k_plus_one(mean_k):
    rng = np.random.default_rng(3); xyz = np.full((2 * mean_k + 7, 3), np.nan, np.float32)
    xyz[rng.permutation(len(xyz))[:mean_k + 1]] = rng.normal(size=(mean_k + 1, 3))
    return cloud(xyz)


def k_finite_among_nans(mean_k):
    rng = np.random.default_rng(4); xyz = np.full((2 * mean_k + 7, 3), np.nan, np.float32)
    xyz[rng.permutation(len(xyz))[:mean_k]] = rng.normal(size=(mean_k, 3))
    return cloud(xyz)


def planar(mean_k=None):
    rng = np.random.default_rng(5); xyz = rng.random((1500, 3)) * (4.0, 3.0, 0.0) + (0.0, 0.0, 2.5)
    xyz[7] = (40.0, 3.0, 2.5)                                           # an outlier inside the plane
    return cloud(xyz)


def collinear(mean_k=None):
    rng = np.random.default_rng(6); x = rng.random(800) * 5.0; x[::9] = x[1::9][:len(x[::9])]      # some coincident pairs
    return cloud(np.stack([x, np.full(800, -1.25), np.full(800, 0.75)], 1))


def offset(mean_k=None):
    rng = np.random.default_rng(8)                                     # FP32 spacing at 1e4 is 2^-10: the coordinates and their differences round
    return cloud(rng.random((2000, 3)) * 2.0 + 1.0e4)


def two_points(mean_k=None):
    """two points, each the other's only neighbour: equal distances d, and at mean_k = 1 the variance (2 fl32(d*d) - (2d)^2 / 2) / 1 is slightly negative: a NaN
    threshold, nothing removed"""
    return cloud(np.random.default_rng(4).normal(size=(2, 3)))


def tiny(n):
    def make(mean_k=None):
        return cloud(np.random.default_rng(n).normal(size=(n, 3)))
    make.__name__ = f"n{n}"
    return make


SCENES = [random_far, lattice, coincident, exactly_k_plus_one, k_finite_among_nans, planar, collinear, offset, two_points] + [tiny(n) for n in (0, 1, 63, 64, 65)]
SCENE = {f.__name__: f for f in SCENES}
CASES = [(f.__name__, k) for f in SCENES for k in MEAN_KS]


@functools.lru_cache(maxsize=None)
def reference(name, mean_k, stddev_mul=1.0):
    """the literal numpy result, computed once per case and shared"""
    return R.filter_outliers(SCENE[name](mean_k), mean_k, stddev_mul)


@functools.lru_cache(maxsize=None)
def twin(name, mean_k, stddev_mul=1.0):
    from sindslam_amd.cloud import filterOutliersHost
    return filterOutliersHost([SCENE[name](mean_k)], mean_k, stddev_mul)[0]


def f64_bytes(*v):
    return np.array(v, np.float64).tobytes()


def assert_equals_reference(got, points, ref):
    """got: a dict of filterOutliers / filterOutliersHost; ref: a dict of cloud_filter_ref.filter_outliers.  Bits, bytes and indices."""
    assert np.array_equal(got["distances"].view(np.uint32), ref["distances"].view(np.uint32))
    assert f64_bytes(got["mean"], got["stddev"], got["threshold"]) == f64_bytes(ref["mean"], ref["stddev"], ref["threshold"])
    assert (got["valid"], got["degenerate"]) == (ref["valid"], ref["degenerate"])
    assert got["points"].tobytes() == points[ref["keep"]].tobytes()


def assert_same(dev, host):
    """device result against the twin's: distances, the stats but the path counters, the bytes of out, n_out"""
    assert np.array_equal(dev["distances"].view(np.uint32), host["distances"].view(np.uint32))
    assert dev["stats"].tobytes()[:32] == host["stats"].tobytes()[:32]
    assert len(dev["points"]) == len(host["points"]) and dev["points"].tobytes() == host["points"].tobytes()
