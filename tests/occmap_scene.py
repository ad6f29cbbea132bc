"""Scenes of the occupancy map's tests (tests/test_occmap_cpu.py, tests/test_occmap_gpu.py) and the comparisons both files use.  A scene is a resolution and a list
of key frames (cloud of POINT_DTYPE, origin); the colours are random unless the scene is about colours.  Every scene is the smallest shape at which its property
shows; the reference state (tests/occmap_ref.py, pure Python) is computed once per scene and shared."""
import functools

import numpy as np

import occmap_ref as R
from sindslam_amd.cloud import POINT_DTYPE

F = np.float32


def cloud(xyz, rgb=None, seed=11):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3); p = np.zeros(len(xyz), POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    c = np.random.default_rng(seed).integers(0, 255, (len(xyz), 3)).astype(np.uint8) if rgb is None else np.asarray(rgb, np.uint8).reshape(-1, 3)
    p["r"], p["g"], p["b"] = c[:, 0], c[:, 1], c[:, 2]; p["a"] = 255
    return p


def axis_aligned():
    """step == 0 on two axes (tMax = DBL_MAX there), all six directions; 0.05"""
    o = (0.51, 0.51, 0.51)
    ends = [(0.93, 0.51, 0.51), (0.02, 0.51, 0.51), (0.51, 0.93, 0.51), (0.51, 0.02, 0.51), (0.51, 0.51, 0.93), (0.51, 0.51, 0.02), (0.51, 0.51, 0.56)]
    return 0.05, [(cloud(ends), o)]


def diagonals():
    """exact diagonals from a voxel centre: tMax ties on two axes and on all three, in every sign pattern with z >= 0 at the end; 0.1"""
    c = 0.55; d = 0.4; ends = []
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if abs(sx) + abs(sy) + abs(sz) >= 2:
                    ends.append((c + sx * d, c + sy * d, c + sz * d))
    return 0.1, [(cloud(ends), (c, c, c))]


def negative():
    """negative coordinates; 0.02"""
    rng = np.random.default_rng(21); ends = rng.random((60, 3)) * (1.0, 1.0, 0.6) + (-1.5, -1.5, 0.0)
    return 0.02, [(cloud(ends), (-1.003, -0.507, 0.31))]


def faces():
    """origins and ends exactly on voxel faces (multiples of the resolution as FP32 fall on either side of the FP64 face; 0.0 and -0.0 are z faces); 0.05 and 0.1"""
    g = np.arange(-4, 5) * 0.05
    ends = [(x, y, z) for x in g[::2] for y in g[1::3] for z in (0.0, -0.0, 0.05, 0.15, 0.35)]
    return 0.05, [(cloud(ends), (0.1, 0.2, 0.0)), (cloud(ends[::3]), (-0.15, 0.0, 0.3))]


def faces_coarse():
    g = np.arange(-3, 4) * 0.1
    ends = [(x, y, z) for x in g for y in g[::2] for z in (0.0, 0.1, 0.3)]
    return 0.1, [(cloud(ends), (0.1, -0.2, 0.2))]


def same_voxel():
    """origin and end in one voxel: the miss list is empty, the voxel only gets hits; 0.02"""
    return 0.02, [(cloud([(0.105, 0.105, 0.105), (0.119, 0.101, 0.1), (0.1, 0.1, 0.1)]), (0.11, 0.11, 0.11))]


def key_limits():
    """coordinates at +-655.36 m on either side of the valid keys; a key frame whose origin has no key (every ray skipped, the colours still run); 0.02"""
    a = [(655.35, 0.01, 0.01), (655.37, 0.01, 0.01), (655.30, 0.01, 0.05), (655.30, 0.01, -0.01), (655.37, 0.01, -0.01)]
    b = [(-655.35, 0.01, 0.01), (-655.37, 0.01, 0.01), (-655.30, -0.01, 0.03)]
    c = [(655.35, 0.01, 0.01), (655.30, 0.01, 0.05), (655.0, 0.0, 0.0)]
    return 0.02, [(cloud(a), (655.25, 0.01, 0.01)), (cloud(b), (-655.28, 0.0, 0.02)), (cloud(c, seed=5), (655.37, 0.01, 0.01))]


@functools.lru_cache(maxsize=None)
def _early_stop_rays():
    """random short rays, scanned with the reference for those whose loop ends by the length test and not by reaching the end key.  Among 4 000 rays with random ends
    there is none; a ray that ends ON a voxel face (one coordinate a multiple of the resolution) must cross that face at t = length, and the FP32 rounding of the
    direction decides on which side of it the last tMax falls."""
    P = R.Params(0.05); rng = np.random.default_rng(33); o = (0.013, -0.021, 0.34); found, other = [], []
    ends = rng.random((400, 3)) * (1.2, 1.2, 0.6) + (-0.6, -0.6, 0.0); axis = rng.integers(0, 3, 400)
    ends[np.arange(400), axis] = np.round(ends[np.arange(400), axis] / 0.05) * 0.05
    for e in ends.astype(np.float32):
        r = R.ray(P, o, e)
        (found if r[2] else other).append(tuple(e))
        if len(found) >= 6:
            break
    return o, found, other[:20]


def early_stop():
    """rays that end by min(tMax) > length; 0.05"""
    o, found, other = _early_stop_rays()
    return 0.05, [(cloud(found + other), o)]


V = (0.55, 0.05, 0.05)                                                  # the voxel the order scenes are about
THROUGH = (0.95, 0.05, 0.05)                                            # a ray from O to here passes through V
O = (0.05, 0.05, 0.05)


def order_hits_then_miss():
    """five hits then a miss in one voxel: 3.5 + miss.  A sum of the updates gives something else; 0.1"""
    return 0.1, [(cloud([V] * 5 + [THROUGH]), O)]


def order_miss_then_hits():
    """a miss then five hits: 3.5"""
    return 0.1, [(cloud([THROUGH] + [V] * 5), O)]


def clamp():
    """eight hits (the clamp holds after five), then sixteen misses (the other clamp after fourteen); beside it one single hit, which sits exactly ON occ_thres; 0.1"""
    return 0.1, [(cloud([V] * 8 + [THROUGH] * 16 + [(0.05, 0.75, 0.05)]), O)]


def many_hits():
    """a voxel with 100 end points and 60 rays through it, interleaved at random: more than one wave's worth of ids in one list; 0.1"""
    rng = np.random.default_rng(44); kind = rng.permutation([0] * 100 + [1] * 60)
    ends = [(0.5 + 0.1 * rng.random(), 0.1 * rng.random(), 0.1 * rng.random()) if k == 0 else (0.95, 0.05 + 0.01 * rng.random(), 0.05) for k in kind]
    return 0.1, [(cloud(ends), O)]


def fan_5000():
    """5 000 short rays from one origin: every one of them a miss on the origin's voxel; 0.02"""
    rng = np.random.default_rng(55); d = rng.normal(size=(5000, 3)); d *= (0.02 + 0.08 * rng.random((5000, 1))) / np.linalg.norm(d, axis=1, keepdims=True)
    return 0.02, [(cloud(d + (0.301, 0.207, 0.2)), (0.301, 0.207, 0.2))]


def colours():
    """successive blends in one voxel; a white point (the voxel stays "not set") and a colour after it; points with z < 0 in a known voxel (the rays from an origin
    below z = 0 made it known) and in an unknown one; NaN and inf points; 0.05"""
    nan, inf = float("nan"), float("inf"); o = (0.02, 0.02, -0.22)
    xyz = [(0.02, 0.02, 0.33), (0.03, 0.03, 0.34), (0.04, 0.01, 0.31), (0.01, 0.04, 0.32),       # four colours into one voxel
           (0.32, 0.02, 0.12),                                                                   # white
           (0.02, 0.02, -0.12), (0.03, 0.01, -0.11),                                             # z < 0, on the first ray's path: known
           (0.52, 0.52, -0.52),                                                                  # z < 0, unknown
           (nan, 0.0, 0.1), (0.1, inf, 0.1), (0.1, 0.1, -inf), (nan, nan, nan),
           (0.02, 0.02, 0.33)]
    rgb = [(10, 200, 30), (250, 0, 7), (0, 0, 0), (100, 100, 100), (255, 255, 255), (9, 8, 7), (200, 100, 50), (1, 2, 3), (5, 5, 5), (6, 6, 6), (7, 7, 7), (8, 8, 8), (254, 255, 255)]
    second = cloud([(0.32, 0.02, 0.12), (0.02, 0.02, -0.12)], [(40, 50, 60), (255, 255, 255)])
    return 0.05, [(cloud(xyz, rgb), o), (second, (0.3, 0.02, 0.3))]


def prune_block():
    """eight sibling voxels driven to the clamp by white points, one key frame each with the origin inside the voxel: octomap prunes them into their parent.  Then one
    coloured point: the pruning tree colours the whole parent, the flat map one voxel -- the contract's second divergence, made visible; 0.1"""
    frames = []
    for k in range(8):
        c = (0.05 + 0.1 * (k & 1), 0.05 + 0.1 * ((k >> 1) & 1), 0.05 + 0.1 * (k >> 2))
        frames.append((cloud([c] * 6, [(255, 255, 255)] * 6), c))
    frames.append((cloud([(0.05, 0.05, 0.05)], [(12, 34, 56)]), (0.05, 0.05, 0.05)))
    return 0.1, frames


def random_mix():
    """three key frames from three origins, NaNs, z < 0 and far points among them: the batch scene; 0.05"""
    rng = np.random.default_rng(66); frames = []
    for f in range(3):
        xyz = rng.random((150, 3)) * (1.6, 1.6, 1.0) + (-0.8, -0.8, -0.2); xyz[::17] = np.nan; xyz[5] = (700.0, 0.0, 0.1)
        frames.append((cloud(xyz, seed=70 + f), tuple(rng.random(3) * 0.4 - (0.2, 0.2, 0.3))))
    return 0.05, frames


def random_fine():
    """the same at 0.02, one key frame"""
    rng = np.random.default_rng(77); xyz = rng.random((120, 3)) * (0.8, 0.8, 0.5) + (-0.4, -0.4, -0.1); xyz[::13] = np.nan
    return 0.02, [(cloud(xyz), (0.013, -0.017, 0.11))]


SCENES = [axis_aligned, diagonals, negative, faces, faces_coarse, same_voxel, key_limits, early_stop, order_hits_then_miss, order_miss_then_hits, clamp, many_hits,
          fan_5000, colours, prune_block, random_mix, random_fine]
SCENE = {f.__name__: f for f in SCENES}
NAMES = [f.__name__ for f in SCENES]
MAX_VOXELS, MAX_POINTS = 1 << 16, 8192


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (FlatMap after all key frames, [stats per key frame], PruneTree fed with the same calls)"""
    res, frames = SCENE[name](); P = R.Params(res); flat = R.FlatMap(P); tree = R.PruneTree(P)
    return flat, [flat.insert(c, o, tree) for c, o in frames], tree


def run(m, name, batch=False):
    """the scene into an OccupancyMap, key frame by key frame or as one batch -> the stats"""
    _, frames = SCENE[name]()
    if batch:
        return list(m.insert([c for c, _ in frames], [o for _, o in frames]))
    return [m.insert([c], [o])[0] for c, o in frames]


def probe_keys(name):
    """the reference's voxels and, around each, the six neighbours (many of them unknown)"""
    flat = reference(name)[0]; keys = set(flat.vox)
    for k in list(flat.vox):
        for a in range(3):
            for d in (-1, 1):
                n = list(k); n[a] += d
                if 0 <= n[a] < 65536:
                    keys.add(tuple(n))
    return np.array(sorted(keys), np.uint16).reshape(-1, 3)


def state(m, name):
    """everything the map shows: read() over probe_keys, size, occupied() as bytes"""
    known, lo, rgb = m.read(probe_keys(name))
    return dict(known=known, logodds=lo.view(np.uint32), rgb=rgb, size=m.size, occupied=m.occupied())


def assert_equals_reference(st, stats, name):
    flat, rstats, _ = reference(name); keys = probe_keys(name); P = flat.P
    for i, k in enumerate(map(tuple, keys.tolist())):
        v = flat.vox.get(k)
        assert st["known"][i] == (v is not None), k
        if v is not None:
            assert st["logodds"][i] == np.float32(v[0]).view(np.uint32) and tuple(st["rgb"][i]) == v[1], (k, st["logodds"][i], v)
        else:
            assert st["logodds"][i] == 0 and not st["rgb"][i].any()
    assert st["size"] == len(flat.vox)
    for g, r in zip(stats, rstats):
        assert {f: int(g[f]) for f in g.dtype.names} == {f: r[f] for f in g.dtype.names}
    occ = flat.occupied(); got = st["occupied"]
    assert len(got) == len(occ)
    want = np.zeros(len(occ), POINT_DTYPE)
    for i, (k, c) in enumerate(occ):
        want[i] = (F(R.coord(P, k[0])), F(R.coord(P, k[1])), F(R.coord(P, k[2])), c[2], c[1], c[0], 0)
    assert got.tobytes() == want.tobytes()


def assert_same(dev, host):
    """device state against the twin's, bit for bit"""
    for f in ("known", "logodds", "rgb"):
        assert np.array_equal(dev[f], host[f]), f
    assert dev["size"] == host["size"] and dev["occupied"].tobytes() == host["occupied"].tobytes()


@functools.lru_cache(maxsize=None)
def twin(name):
    """the host twin's state and stats after the scene, computed once"""
    from sindslam_amd.occupancy import OccupancyMap
    res, _ = SCENE[name](); m = OccupancyMap(res, max_voxels=MAX_VOXELS, max_points=MAX_POINTS, host=True)
    stats = run(m, name); st = state(m, name); m.close()
    return st, stats
