"""Scenes of the snapshot tree's tests (tests/test_occmap_tree_cpu.py, tests/test_occmap_tree_gpu.py) and the comparisons both files use.  A scene is a resolution and a
list of key frames (cloud, origin).  Each is the smallest shape at which its property shows; what is
slow in pure Python (the flat reference map of a scene) is computed once per scene and shared."""
import functools

import numpy as np

import occmap_ref as R
import occmap_tree_ref as T
from occmap_scene import cloud
from sindslam_amd.cloud import POINT_DTYPE

F = np.float32
SETTINGS = [(0, 0), (0, 1), (1, 0), (1, 1)]                             # (prune, inner_colour)
MAX_VOXELS, MAX_POINTS = 1 << 14, 4096


def _shell(res, half, shift):
    """points on the six faces of a cube of half-side `half` voxels, one per face voxel, seen from an origin near its centre (the points with z < 0 cast no ray, so
    the known voxels are the upper half); the same key frame five times, so that a voxel inside that lies on one ray only still reaches clamp_min (5 misses of -0.405
    against -2.0) and stays white: free space that prunes"""
    g = (np.arange(-np.floor(half), np.floor(half) + 1)) * res; pts = []
    for a in range(3):
        for s in (-1, 1):
            for u in g:
                for v in g:
                    p = [0.0, 0.0, 0.0]; p[a] = s * half * res; p[(a + 1) % 3] = u + 0.013; p[(a + 2) % 3] = v + 0.011
                    pts.append(p)
    xyz = np.array(pts) + shift; o = tuple(np.array((0.03, 0.02, 0.01)) + shift)
    return res, [(cloud(xyz, seed=3), o)] * 5


def shell():
    """0.25, half-side 8.5 voxels: leaves at depths 13 and 16"""
    return _shell(0.25, 8.5, (0.0, 0.0, 0.0))


def shell_shifted():
    """the same, moved by (0.6, 0.3, 0): leaves at depths 13, 14, 15 and 16"""
    return _shell(0.25, 8.5, (0.6, 0.3, 0.0))


def shell_small():
    """0.1, half-side 6.3 voxels: leaves at depths 14, 15 and 16"""
    return _shell(0.1, 6.3, (0.0, 0.0, 0.0))


COLOURS = [(200, 40, 90), (10, 220, 30), (0, 0, 0), (90, 90, 250), (120, 60, 20)]


def _hit_only(res, voxels, colours=None, hits=None):
    """per voxel (i, j, k) five key frames of one point: origin and end point inside the voxel, so the miss list is empty; colours(v) / hits(v) override per voxel"""
    frames = []
    for v in voxels:
        c = np.array([(v[0] + 0.5) * res, (v[1] + 0.5) * res, (v[2] + 0.5) * res]); seq = colours(v) if colours else COLOURS
        for f in range(hits(v) if hits else 5):
            frames.append((cloud([c + 0.1 * res], [seq[f]]), tuple(c)))
    return res, frames


def _block(n):
    return [(x, y, z) for z in range(n) for y in range(n) for x in range(n)]


def block8():
    """eight siblings, each at clamp_max with the same blended colour: one occupied depth-15 leaf"""
    return _hit_only(0.1, _block(2))


def block64():
    """the same one level up: one occupied depth-14 leaf"""
    return _hit_only(0.1, _block(4))


def near_missing():
    """isNodeCollapsible, clause 1: one sibling missing"""
    return _hit_only(0.1, _block(2)[:-1])


def near_missing_first():
    """... and child 0 missing (the clause octomap tests first)"""
    return _hit_only(0.1, _block(2)[1:])


def near_colour():
    """clause 3: one sibling's colour one step off"""
    return _hit_only(0.1, _block(2), colours=lambda v: COLOURS[:4] + [(170, 60, 20)] if v == (1, 0, 1) else COLOURS)


def near_value():
    """clause 3: one sibling one hit short, so the values differ.  Four hits stay below clamp_max; its last colour is the others' last, but the blend differs too"""
    return _hit_only(0.1, _block(2), hits=lambda v: 4 if v == (0, 1, 1) else 5, colours=lambda v: COLOURS[1:] if v == (0, 1, 1) else COLOURS)


def near_inner():
    """clause 2: seven leaves and one inner child: a 4 x 4 x 4 block with one voxel missing leaves its parent seven pruned children and one unpruned"""
    return _hit_only(0.1, [v for v in _block(4) if v != (3, 2, 1)])


def one_voxel():
    """one voxel: 17 nodes"""
    return _hit_only(0.1, [(0, 0, 0)])


def empty():
    """the empty map: 0 nodes, no root, a header only"""
    return 0.1, []


def white_only():
    """white points only: inner_colour = 1 stays white everywhere"""
    rng = np.random.default_rng(5); xyz = rng.random((40, 3)) * (0.8, 0.8, 0.4) + (-0.4, -0.4, 0.0)
    return 0.1, [(cloud(xyz, [(255, 255, 255)] * 40), (0.01, 0.02, 0.13))]


def random_cloud():
    """a few hundred random points at 0.1 in two key frames: inner_colour = 1 averages over set and unset children at every level"""
    rng = np.random.default_rng(8); frames = []
    for f in range(2):
        xyz = rng.random((150, 3)) * (1.8, 1.8, 0.9) + (-0.9, -0.9, -0.1)
        frames.append((cloud(xyz, seed=90 + f), (0.02 - 0.3 * f, 0.01, 0.2)))
    return 0.1, frames


SCENES = [shell, shell_shifted, shell_small, block8, block64, near_missing, near_missing_first, near_colour, near_value, near_inner, one_voxel, empty, white_only,
          random_cloud]
SCENE = {f.__name__: f for f in SCENES}
NAMES = [f.__name__ for f in SCENES]


@functools.lru_cache(maxsize=None)
def reference_flat(name, with_prune_tree=False):
    """the pure-Python flat map after the scene (and, if asked, occmap_ref.PruneTree fed with the same calls: slow, one test needs it)"""
    res, frames = SCENE[name](); P = R.Params(res); flat = R.FlatMap(P); tree = R.PruneTree(P) if with_prune_tree else None
    for c, o in frames:
        flat.insert(c, o, tree)
    return flat, tree


def fill(m, name):
    """the scene into an OccupancyMap, as one batch per 64 key frames"""
    _, frames = SCENE[name]()
    for i in range(0, len(frames), 64):
        m.insert([c for c, _ in frames[i:i + 64]], [o for _, o in frames[i:i + 64]])
    return m


def new_map(name, host, **kw):
    from sindslam_amd.occupancy import OccupancyMap
    return OccupancyMap(SCENE[name]()[0], **dict(dict(max_voxels=MAX_VOXELS, max_points=MAX_POINTS, host=host), **kw))


def all_keys(name):
    """the reference's voxels and, around each, the six neighbours (many of them unknown)"""
    keys = set(reference_flat(name)[0].vox)
    for k in list(keys):
        for a in range(3):
            for d in (-1, 1):
                n = list(k); n[a] += d; keys.add(tuple(n))
    return np.array(sorted(keys), np.uint16).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def reference_tree(name, prune, inner_colour):
    """the literal Python tree over the literal Python flat map -> dict(stats, data, leaves [occupied_only] as (points, depth))"""
    t = T.Tree(reference_flat(name)[0], bool(prune), bool(inner_colour)); leaves = {}
    for occ in (0, 1):
        ls = t.leaves(bool(occ)); pts = np.zeros(len(ls), POINT_DTYPE)
        for i, (x, y, z, c, d) in enumerate(ls):
            pts[i] = (x, y, z, c[2], c[1], c[0], 0)
        leaves[occ] = (pts, np.array([l[4] for l in ls], np.uint8))
    return dict(stats=t.stats(), data=t.stream(), leaves=leaves, ot=t.ot())


def assert_tree_equals_reference(m, name, prune, inner_colour):
    """m.tree() against the literal Python tree, byte for byte: stats, stream, leaves (position bits, colour, depth) for both occupied_only settings"""
    ref = reference_tree(name, prune, inner_colour)
    for occ in (0, 1):
        got = m.tree(prune, inner_colour, occupied_only=occ); st = got["stats"]
        assert {f: (st[f].tolist() if f == "leaves_at_depth" else int(st[f])) for f in st.dtype.names} == ref["stats"], (name, prune, inner_colour)
        assert got["data"].tobytes() == ref["data"] and len(got["data"]) == 8 * ref["stats"]["n_nodes"]
        assert got["leaves"].tobytes() == ref["leaves"][occ][0].tobytes() and got["depth"].tobytes() == ref["leaves"][occ][1].tobytes()
    return ref


def same_tree(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in ("stats", "data", "leaves", "depth"))
