"""GPU: sind_occmap_tree / sind_occmap_write_ot (csrc/occmap_tree.hip: a hash table of inner nodes, one kernel per level up with integer atomics, one per level down)
against the host twin and the literal Python tree of tests/occmap_tree_ref.py, byte for byte: the writeData stream, the stats, the leaves.  The three share the contract
and nothing of the schedule: Python and the twin recurse over a pointer tree, the device sweeps levels.  The twin and the Python tree are pinned to each other by
tests/test_occmap_tree_cpu.py.  Parity with a real octomap build is unpinned."""
import ctypes as C

import numpy as np
import pytest

import occmap_tree_ref as T
import occmap_tree_scene as S

pytestmark = pytest.mark.gpu

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
KEYS = ("imgRGB", "imgDepth", "imgDepthLast", "imgDynaMask", "imgDynaMaskLast", "imgLabel", "poseRelative", "Twc")


def _state(m, name):
    return m.size, m.occupied().tobytes(), [a.tobytes() for a in m.read(S.all_keys(name))]


@pytest.mark.parametrize("name", S.NAMES)
def test_device_equals_the_twin_and_the_literal_tree(name):
    """every (prune, inner_colour) setting, both occupied_only settings; two calls in a row return identical bytes; the map is unchanged by all of it"""
    d = S.fill(S.new_map(name, False), name); h = S.fill(S.new_map(name, True), name)
    before = _state(d, name); assert before == _state(h, name)
    for pr, ic in S.SETTINGS:
        S.assert_tree_equals_reference(d, name, pr, ic)
        for occ in (0, 1):
            a, b, t = d.tree(pr, ic, occ), d.tree(pr, ic, occ), h.tree(pr, ic, occ)
            assert S.same_tree(a, b) and S.same_tree(a, t)
        assert d.size_nodes(pr) == S.reference_tree(name, pr, ic)["stats"]["n_nodes"] and d.full_map_msg(pr, ic)["data"] == S.reference_tree(name, pr, ic)["data"]
    leaves, depth = d.leaves(prune=False, occupied_only=True)
    assert leaves.tobytes() == d.occupied().tobytes() and (depth == 16).all()
    assert _state(d, name) == before
    d.close(); h.close()


@pytest.mark.parametrize("name", ["shell_shifted", "block64", "near_inner", "random_cloud", "empty"])
def test_the_ot_file_parses_back_to_a_read_of_its_own_leaves(name, tmp_path):
    d = S.fill(S.new_map(name, False), name)
    for pr, ic in S.SETTINGS:
        path = tmp_path / f"{pr}{ic}.ot"; d.write_ot(str(path), pr, ic); blob = path.read_bytes()
        assert blob == S.reference_tree(name, pr, ic)["ot"]
        tid, size, res, leaves = T.parse_ot(blob); vox = T.expand(leaves)
        assert tid == "ColorOcTree" and size == d.size_nodes(pr) and res == d.resolution and len(vox) == d.size
        if vox:
            keys = np.array(sorted(vox), np.uint16); known, lo, rgb = d.read(keys)
            assert known.all() and [(int(b), tuple(int(v) for v in c)) for b, c in zip(lo.view(np.uint32), rgb)] == [vox[tuple(k)] for k in keys.tolist()]
    d.close()


def test_capacity_with_the_counts_filled():
    from sindslam_amd._lib import lib, ptr
    from sindslam_amd.cloud import POINT_DTYPE
    from sindslam_amd.occupancy import TREE_STATS_DTYPE, OccupancyMap
    L = lib(); name = "shell_small"; d = S.fill(S.new_map(name, False), name); ref = S.reference_tree(name, 1, 0)
    n, nl, nocc = ref["stats"]["n_nodes"], ref["stats"]["n_leaves"], ref["stats"]["n_occupied_leaves"]
    st = np.zeros(1, TREE_STATS_DTYPE); cnt = np.zeros(1, np.int32); data = np.full(8 * n, 7, np.uint8); leaves = np.zeros(nl, POINT_DTYPE); depth = np.full(nl, 99, np.uint8)
    assert L.sind_occmap_tree(d._h, 1, 0, 0, None, C.c_size_t(0), None, None, 0, None, None) == SIND_E_ARG and L.sind_last_error()
    assert L.sind_occmap_tree(d._h, 1, 0, 0, None, C.c_size_t(0), None, ptr(depth), 0, None, ptr(st)) == SIND_E_ARG
    assert L.sind_occmap_tree(d._h, 1, 0, 0, ptr(data), C.c_size_t(8 * n - 1), None, None, 0, ptr(cnt), ptr(st)) == SIND_E_CAPACITY and b"capacity" in L.sind_last_error()
    assert st[0]["n_nodes"] == n and st[0]["leaves_at_depth"].tolist() == ref["stats"]["leaves_at_depth"] and cnt[0] == nl and (data == 7).all()
    st[:] = 0; cnt[:] = 0
    assert L.sind_occmap_tree(d._h, 1, 0, 1, ptr(data), C.c_size_t(8 * n), ptr(leaves), ptr(depth), nocc - 1, ptr(cnt), ptr(st)) == SIND_E_CAPACITY
    assert st[0]["n_occupied_leaves"] == nocc == cnt[0] and (data == 7).all() and (depth == 99).all()
    assert L.sind_occmap_tree(d._h, 1, 0, 1, ptr(data), C.c_size_t(8 * n), ptr(leaves), None, nocc, ptr(cnt), ptr(st)) == 0      # exactly enough; the depths are optional
    assert data.tobytes() == ref["data"] and leaves[:nocc].tobytes() == ref["leaves"][1][0].tobytes() and (depth == 99).all()
    assert L.sind_occmap_write_ot(d._h, 1, 0, None) == SIND_E_ARG and L.sind_occmap_write_ot(d._h, 1, 0, b"/nonexistent-directory/x.ot") == SIND_E_ARG
    d.close()
    # the limit on inner nodes: max_voxels = 256 gives 1024 slots and so 512 inner nodes.  Scattered voxels share few ancestors: 50 of them need 497, 60 need 588
    import occmap_ref as R
    from occmap_scene import cloud
    rng = np.random.default_rng(12); k = rng.integers(-2048, 2048, (60, 3)); k[:, 2] = np.abs(k[:, 2]); c = (k + 0.5) * 0.1
    frames = [(cloud([p + 0.01], [(9, 8, 7)]), tuple(p)) for p in c]; flat = R.FlatMap(R.Params(0.1))
    m = OccupancyMap(0.1, max_voxels=256, max_points=16); t = OccupancyMap(0.1, max_voxels=256, max_points=16, host=True)
    for x in (m, t):
        x.insert([f[0] for f in frames[:50]], [f[1] for f in frames[:50]])
    for f in frames[:50]:
        flat.insert(*f)
    inner = T.Tree(flat, True).stats()["n_inner"]; assert 480 < inner <= 512
    assert S.same_tree(m.tree(), t.tree()) and m.tree()["stats"]["n_inner"] == inner
    m.insert([f[0] for f in frames[50:]], [f[1] for f in frames[50:]]); assert m.size == 60
    for f in frames[50:]:
        flat.insert(*f)
    assert T.Tree(flat, True).stats()["n_inner"] > 512
    before = m.occupied().tobytes()
    assert L.sind_occmap_tree(m._h, 1, 0, 0, None, C.c_size_t(0), None, None, 0, None, ptr(st)) == SIND_E_CAPACITY and b"inner nodes" in L.sind_last_error()
    assert m.size == 60 and m.occupied().tobytes() == before
    m.clear(); m.insert([f[0] for f in frames[:50]], [f[1] for f in frames[:50]]); assert S.same_tree(m.tree(), t.tree())      # and the workspace recovers
    m.close(); t.close()


def test_a_tree_an_insert_and_a_tree_again():
    """the snapshot keeps nothing between calls: tree, insert, tree equals the tree of a map that got both inserts"""
    name = "random_cloud"; _, frames = S.SCENE[name]()
    a = S.new_map(name, False); b = S.new_map(name, False); h = S.new_map(name, True)
    a.insert([frames[0][0]], [frames[0][1]]); first = a.tree(True, True)
    h.insert([frames[0][0]], [frames[0][1]]); assert S.same_tree(first, h.tree(True, True))
    a.insert([frames[1][0]], [frames[1][1]]); second = a.tree(True, True)
    S.fill(b, name)
    assert S.same_tree(second, b.tree(True, True)) and not first["data"].tobytes() == second["data"].tobytes()
    S.assert_tree_equals_reference(a, name, 1, 1)
    a.clear(); assert a.size_nodes() == 0 and len(a.tree()["data"]) == 0
    a.close(); b.close(); h.close()


def test_a_stream_keyframe_inserted_where_generate_left_it(stream):
    """insertGenerated of one stream key frame (more than 30 000 points) at 0.02, then the tree of the device against the twin's on the downloaded cloud: more than
    100 000 voxels, leaves at several depths"""
    import cloud_scene as CS
    from sindslam_amd.cloud import CloudGenerator
    from sindslam_amd.occupancy import OccupancyMap
    cam5, a = CS.keyframe_pair(stream, 8, 2); g = CloudGenerator(*cam5, max_batch=1)
    args = [a[k][None] for k in KEYS]; Twc = args[-1]
    cloud = g.generatePointCloud(*args)[0]["points"]
    d = OccupancyMap(0.02, max_voxels=1 << 21, max_points=g.cap); h = OccupancyMap(0.02, max_voxels=1 << 21, max_points=g.cap, host=True)
    d.insertGenerated(g, Twc); h.insert([cloud], Twc[:, :3, 3].astype(np.float32))
    assert d.size == h.size > 100000
    got = []
    for pr, ic, occ in ((1, 0, 1), (0, 1, 0)):
        x, y = d.tree(pr, ic, occ), h.tree(pr, ic, occ); got.append(x)
        assert S.same_tree(x, y) and len(x["data"]) == 8 * x["stats"]["n_nodes"]
    st, flat = got[0]["stats"], got[1]["stats"]
    assert st["n_pruned"] > 1000 and (st["leaves_at_depth"] > 0).sum() >= 3 and st["n_leaves"] == st["leaves_at_depth"].sum() and st["n_nodes"] < flat["n_nodes"]
    assert flat["n_leaves"] == d.size and len(got[0]["leaves"]) == st["n_occupied_leaves"] and len(got[1]["leaves"]) == d.size
    g.close(); d.close(); h.close()
