"""GPU: sind_occmap_* (csrc/occmap_kernels.hip) against the host twin, bit for bit: the known flags, the log-odds bits, the colours, the stats, size and the occupied
list with its order.  The twin is pinned to the literal contract by tests/test_occmap_cpu.py; the two share the arithmetic (csrc/host/occmap.hpp) and nothing of the
schedule: the twin runs the sequential loops, the device counts misses per gap with integer atomics and replays each voxel."""
import ctypes as C

import numpy as np
import pytest

import occmap_scene as S

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_STATE, SIND_E_CAPACITY = -1, -4, -5
KEYS = ("imgRGB", "imgDepth", "imgDepthLast", "imgDynaMask", "imgDynaMaskLast", "imgLabel", "poseRelative", "Twc")


def _map(res, **kw):
    from sindslam_amd.occupancy import OccupancyMap
    return OccupancyMap(res, **dict(dict(max_voxels=S.MAX_VOXELS, max_points=S.MAX_POINTS), **kw))


def _same_stats(dev, host):
    assert [tuple(int(v) for v in s) for s in dev] == [tuple(int(v) for v in s) for s in host]


@pytest.mark.parametrize("name", S.NAMES)
def test_device_equals_the_twin_twice(name):
    """twice on a cleared map: the slots a second run gets differ (the claims race), nothing visible may"""
    host, hstats = S.twin(name); m = _map(S.SCENE[name]()[0])
    for _ in range(2):
        _same_stats(S.run(m, name), hstats)
        S.assert_same(S.state(m, name), host)
        m.clear(); assert m.size == 0 and len(m.occupied()) == 0
    m.close()


@pytest.mark.parametrize("name", ["random_mix", "colours", "key_limits", "prune_block"])
def test_a_batch_equals_the_calls_in_order(name):
    host, hstats = S.twin(name); m = _map(S.SCENE[name]()[0])
    _same_stats(S.run(m, name, batch=True), hstats)
    S.assert_same(S.state(m, name), host); m.close()


def test_accumulation_over_two_calls_and_a_batch_with_an_empty_cloud():
    res, frames = S.SCENE["random_mix"](); empty = frames[0][0][:0]
    clouds = [frames[0][0], empty, frames[1][0]]; origins = [frames[0][1], (0.0, 0.0, 0.0), frames[1][1]]
    d = _map(res); h = _map(res, host=True)
    for m in (d, h):
        m.insert([frames[2][0]], [frames[2][1]])                       # call 1
    sd, sh = d.insert(clouds, origins), h.insert(clouds, origins)      # call 2 accumulates on it
    _same_stats(sd, sh); assert not any(sd[1]) and sd[0]["n_rays"] > 0
    S.assert_same(S.state(d, "random_mix"), S.state(h, "random_mix"))
    assert d.size == S.twin("random_mix")[0]["size"]                   # the same voxels as the scene's order of key frames; the values differ, order matters
    d.close(); h.close()


def test_points_on_the_device_with_a_stride():
    import torch
    from sindslam_amd._lib import check, lib, ptr
    from sindslam_amd.cloud import POINT_DTYPE
    from sindslam_amd.occupancy import OCC_STATS_DTYPE
    res, frames = S.SCENE["random_mix"](); stride = 333; n = np.array([len(c) for c, _ in frames], np.int32)
    pts = np.zeros((3, stride), POINT_DTYPE)
    for b, (c, _) in enumerate(frames):
        pts[b, :len(c)] = c
    pts[:, 200:]["x"] = 1.0; pts[:, 200:]["z"] = 1.0                   # beyond n_points: must not be read as points
    dpts = torch.from_numpy(pts.view(np.uint8).reshape(3, stride * 16).copy()).cuda(); torch.cuda.synchronize()
    org = np.array([o for _, o in frames], np.float32); st = np.zeros(3, OCC_STATS_DTYPE); m = _map(res)
    check(lib().sind_occmap_insert(m._h, 3, ptr(int(dpts.data_ptr())), stride, ptr(n), ptr(org), 1, ptr(st)))
    host, hstats = S.twin("random_mix")
    _same_stats(st, hstats); S.assert_same(S.state(m, "random_mix"), host); m.close()


def test_errors_and_capacity():
    from sindslam_amd._lib import lib, ptr
    from sindslam_amd.cloud import POINT_DTYPE
    from sindslam_amd.occupancy import OCC_STATS_DTYPE
    L = lib(); h = C.c_void_p(); d = C.c_double
    create = lambda res, ph, pm, c0, c1, occ, mv, mp: L.sind_occmap_create(d(res), d(ph), d(pm), d(c0), d(c1), d(occ), mv, mp, 0, C.byref(h))
    for bad in ((0.0, .7, .4, .1192, .971, .7, 10, 10), (0.02, 1.0, .4, .1192, .971, .7, 10, 10), (0.02, .7, .4, .971, .1192, .7, 10, 10), (0.02, .7, .4, .1192, .971, .7, 0, 10),
                (1e-9, .7, .4, .1192, .971, .7, 10, 10)):
        assert create(*bad) == SIND_E_ARG and L.sind_last_error()
    assert create(0.02, .7, .4, .1192, .971, .7, (1 << 26) + 1, 10) == SIND_E_CAPACITY
    res, frames = S.SCENE["random_mix"](); need = []
    t = _map(res, host=True)
    for c, o in frames:
        t.insert([c], [o]); need.append(t.size)
    t.close()
    m = _map(res, max_voxels=need[1]); m.insert([frames[0][0]], [frames[0][1]]); m.insert([frames[1][0]], [frames[1][1]]); assert m.size == need[1]      # exactly enough
    m.close()
    m = _map(res, max_voxels=need[1] - 1); t = _map(res, max_voxels=need[1] - 1, host=True)
    for x in (m, t):
        x.insert([frames[0][0]], [frames[0][1]])
    before = S.state(m, "random_mix")
    pts = np.ascontiguousarray(frames[1][0]); n = np.array([len(pts)], np.int32); org = np.array(frames[1][1], np.float32); st = np.full(1, 7, OCC_STATS_DTYPE)
    assert L.sind_occmap_insert(m._h, 1, ptr(pts), len(pts), ptr(n), ptr(org), 0, ptr(st)) == SIND_E_CAPACITY and b"max_voxels" in L.sind_last_error()
    S.assert_same(S.state(m, "random_mix"), before); S.assert_same(before, S.state(t, "random_mix")); assert not any(st[0])      # one voxel too many: the map as it was
    small = frames[1][0][:3]                                            # after the refusal a key frame that fits goes in, on both sides alike
    _same_stats(m.insert([small], [frames[1][1]]), t.insert([small], [frames[1][1]])); S.assert_same(S.state(m, "random_mix"), S.state(t, "random_mix"))
    # in a batch the key frames before the refused one are in the map
    m.clear(); t.clear()
    with pytest.raises(Exception):
        m.insert([c for c, _ in frames], [o for _, o in frames])
    t.insert([frames[0][0]], [frames[0][1]])
    S.assert_same(S.state(m, "random_mix"), S.state(t, "random_mix")); assert m.size == need[0]
    # arguments
    assert L.sind_occmap_insert(m._h, 1, ptr(pts), len(pts) - 1, ptr(n), ptr(org), 0, None) == SIND_E_ARG
    assert L.sind_occmap_insert(m._h, 0, ptr(pts), len(pts), ptr(n), ptr(org), 0, None) == SIND_E_ARG
    assert L.sind_occmap_insert(m._h, 1, ptr(pts), len(pts), ptr(n), ptr(np.array([np.inf, 0, 0], np.float32)), 0, None) == SIND_E_ARG
    big = np.zeros(S.MAX_POINTS + 1, POINT_DTYPE)
    assert L.sind_occmap_insert(m._h, 1, ptr(big), len(big), ptr(np.array([len(big)], np.int32)), ptr(org), 0, None) == SIND_E_CAPACITY
    assert m.size == need[0]
    nocc = np.zeros(1, np.int32); out = np.zeros(1, POINT_DTYPE)
    assert L.sind_occmap_occupied(m._h, ptr(out), 0, ptr(nocc)) == SIND_E_CAPACITY and nocc[0] == len(t.occupied()) > 1
    # insert_generated before any sind_cloud_generate on the cloud handle
    from sindslam_amd.cloud import CloudGenerator
    g = CloudGenerator(525.0, 525.0, 319.5, 239.5, 5000.0, width=64, height=48, max_batch=1)
    assert L.sind_occmap_insert_generated(m._h, g._h, 1, ptr(org), None) == SIND_E_STATE
    g.close(); m.close(); t.close()


def test_stream_keyframes_inserted_where_generate_left_them(stream):
    """insertGenerated after generatePointCloud on the two stream key frames (more than 30 000 points each, NaNs among them) at 0.02, against the twin on the downloaded
    clouds; and generatePointCloud after it still equals the oracle."""
    import oracle_lib as O
    import cloud_scene as CS
    from sindslam_amd.cloud import CloudGenerator
    scenes = [CS.keyframe_pair(stream, t, gap) for t, gap in ((8, 2), (12, 1))]
    cam5 = scenes[0][0]; g = CloudGenerator(*cam5, max_batch=2)
    args = [np.stack([s[1][k] for s in scenes]) for k in KEYS]; Twc = args[-1]
    res = g.generatePointCloud(*args); clouds = [r["points"] for r in res]
    d = _map(0.02, max_voxels=1 << 21, max_points=g.cap); h = _map(0.02, max_voxels=1 << 21, max_points=g.cap, host=True)
    sd = d.insertGenerated(g, Twc); sh = h.insert(clouds, Twc[:, :3, 3].astype(np.float32))
    _same_stats(sd, sh)
    assert all(len(c) > 30000 and np.isnan(c["x"]).any() for c in clouds) and all(s["n_rays"] > 20000 and s["n_miss_updates"] > 10 * s["n_rays"] for s in sd)
    od, oh = d.occupied(), h.occupied()
    assert d.size == h.size > 100000 and len(od) > 10000 and od.tobytes() == oh.tobytes()
    rng = np.random.default_rng(1); k = np.round(np.stack([oh["x"], oh["y"], oh["z"]], 1).astype(np.float64) / 0.02 - 0.5).astype(np.int64) + 32768
    keys = np.concatenate([k, k[rng.integers(0, len(k), 20000)] + rng.integers(-6, 7, (20000, 3))]).astype(np.uint16)      # the occupied voxels and free / unknown ones near them
    for a, b in zip(d.read(keys), h.read(keys)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    again = g.generatePointCloud(*args)
    for got, (_, a) in zip(again, scenes):
        want = O.generate_point_cloud(cam5, *[a[k] for k in KEYS])
        assert got["points"].tobytes() == want["points"].tobytes() and np.array_equal(got["kept"], want["kept"]) and np.array_equal(got["occlusion"], want["occlusion"])
    g.close(); d.close(); h.close()
