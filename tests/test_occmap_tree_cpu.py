"""CPU: the host twin sindh_occmap_tree / sindh_occmap_write_ot (csrc/host/occmap_tree.cpp: a pointer tree, octomap's recursive prune(), updateInnerOccupancy and
writeNodesRecurs) against the literal Python restatement in tests/occmap_tree_ref.py over the literal Python flat map of tests/occmap_ref.py: the writeData stream, the
stats, the leaves (position bits, colour, depth), the .ot file.  The contract is restated from octomap 1.9 as recalled; parity with a real octomap build is unpinned,
and nothing here claims it."""
import os
import struct
import subprocess

import numpy as np
import pytest

import occmap_ref as R
import occmap_scene as S0
import occmap_tree_ref as T
import occmap_tree_scene as S
from sindslam_amd.cloud import POINT_DTYPE
from sindslam_amd.occupancy import TREE_STATS_DTYPE, OccupancyMap

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
FNV0, FNVP, M64 = 1469598103934665603, 1099511628211, (1 << 64) - 1


@pytest.fixture(scope="module")
def twins():
    """the twin's map after each scene, built once and never changed by a tree call (which this module also checks)"""
    maps = {name: S.fill(S.new_map(name, True), name) for name in S.NAMES}
    yield maps
    for m in maps.values():
        m.close()


def _depths(name, prune=1):
    return {d for d, c in enumerate(S.reference_tree(name, prune, 0)["stats"]["leaves_at_depth"]) if c}


def test_the_scenes_are_what_they_claim():
    """the properties the scenes exist for, from the Python reference alone"""
    assert _depths("shell") == {13, 16} and _depths("shell_shifted") == {13, 14, 15, 16} and _depths("shell_small") == {14, 15, 16}
    assert len(S.reference_flat("shell")[0].vox) > 2500 and len(S.reference_flat("shell_small")[0].vox) > 1000
    for name in S.NAMES:
        assert _depths(name, 0) <= {16}
    P = R.Params(0.1)
    # the occupied, coloured pruned leaf, and the same one level up
    for name, n, depth, nodes, centre in (("block8", 8, 15, 16, 0.1), ("block64", 64, 14, 15, 0.2)):
        flat = S.reference_flat(name)[0]; vals = {(float(v[0]), v[1]) for v in flat.vox.values()}; st = S.reference_tree(name, 1, 0)["stats"]
        assert len(flat.vox) == n and len(vals) == 1 and next(iter(vals))[0] == float(P.cmax) >= float(P.occ) and next(iter(vals))[1] != R.WHITE
        assert st["n_nodes"] == nodes and st["n_leaves"] == 1 and st["leaves_at_depth"][depth] == 1 and st["n_occupied_leaves"] == 1 and st["n_pruned"] == (n - 1) // 7
        (x, y, z, c, d), = T.Tree(flat, True).leaves(True)
        assert d == depth and c == next(iter(vals))[1] and x == y == z == np.float32(centre)      # the centre of the block
    # every clause of isNodeCollapsible, one step away
    for name in ("near_missing", "near_missing_first", "near_colour", "near_value"):
        st = S.reference_tree(name, 1, 0)["stats"]; assert st["n_pruned"] == 0 and st["n_nodes"] == S.reference_tree(name, 0, 0)["stats"]["n_nodes"]
    assert len(S.reference_flat("near_missing")[0].vox) == 7 and (32768, 32768, 32768) not in S.reference_flat("near_missing_first")[0].vox
    flat = S.reference_flat("near_colour")[0]; odd = flat.vox[(32769, 32768, 32769)]; rest = {tuple(v) for k, v in flat.vox.items() if k != (32769, 32768, 32769)}
    assert len(flat.vox) == 8 and len(rest) == 1
    (v, c), = rest
    assert odd[0] == v and sorted(abs(a - b) for a, b in zip(odd[1], c)) == [0, 0, 1]                                # equal values, one channel one step off
    flat = S.reference_flat("near_value")[0]; odd = flat.vox[(32768, 32769, 32769)]
    assert len(flat.vox) == 8 and odd[0] < P.cmax and all(v[0] == P.cmax for k, v in flat.vox.items() if k != (32768, 32769, 32769))
    st = S.reference_tree("near_inner", 1, 0)["stats"]
    assert st["n_pruned"] == 7 and st["leaves_at_depth"][15] == 7 and st["leaves_at_depth"][16] == 7 and st["leaves_at_depth"][14] == 0      # seven leaves and one inner child
    t = T.Tree(S.reference_flat("near_inner")[0], True)
    kids = t.root
    while sum(x is not None for x in kids.ch) == 1:
        kids = next(x for x in kids.ch if x is not None)
    assert sum(x is not None and not x.has_children() for x in kids.ch) == 7 and sum(x is not None and x.has_children() for x in kids.ch) == 1 and not T.Tree.collapsible(kids)
    # basic cases
    assert S.reference_tree("one_voxel", 1, 0)["stats"]["n_nodes"] == 17 and S.reference_tree("one_voxel", 1, 0)["stats"]["n_inner"] == 16
    assert S.reference_tree("empty", 1, 1)["stats"]["n_nodes"] == 0 and S.reference_tree("empty", 1, 1)["data"] == b""
    for pr, ic in S.SETTINGS:
        data = S.reference_tree("white_only", pr, ic)["data"]
        assert len(data) > 800 and all(data[i + 4:i + 7] == b"\xff\xff\xff" for i in range(0, len(data), 8))
    # inner_colour = 1 over mixed children: some inner node averages over fewer children than it has, and some inner node is coloured
    t = T.Tree(S.reference_flat("random_cloud")[0], True, True); mixed = coloured = 0
    for n, d, _ in t.walk():
        if n.has_children():
            kids = [c for c in n.ch if c is not None]; ns = sum(c.c != R.WHITE for c in kids)
            mixed += 0 < ns < len(kids); coloured += n.c != R.WHITE
    assert mixed > 20 and coloured > 100
    assert S.reference_tree("random_cloud", 1, 1)["data"] != S.reference_tree("random_cloud", 1, 0)["data"]
    # the root is never pruned.  No flat map can show it (eight depth-1 leaves would take 8 ** 16 voxels), so the tree is made by hand: a root over eight equal leaves
    t = T.Tree(R.FlatMap(P)); t.root = T.Node(); t.root.ch = [T.Node() for _ in range(8)]
    assert T.Tree.collapsible(t.root)
    t.prune(); assert t.n_pruned == 0 and t.stats()["n_nodes"] == 9


@pytest.mark.parametrize("name", S.NAMES)
def test_twin_equals_the_literal_tree(name, twins):
    """stream, stats and leaves for all four (prune, inner_colour) settings and both occupied_only settings, byte for byte; the map is unchanged by it"""
    m = twins[name]; flat = S.reference_flat(name)[0]
    assert m.size == len(flat.vox)
    before = m.size, m.occupied().tobytes(), [a.tobytes() for a in m.read(S.all_keys(name))]
    for pr, ic in S.SETTINGS:
        ref = S.assert_tree_equals_reference(m, name, pr, ic)
        assert m.full_map_msg(pr, ic) == dict(id="ColorOcTree", resolution=flat.P.res, binary=False, data=ref["data"])
        assert m.size_nodes(pr) == ref["stats"]["n_nodes"]
    assert before == (m.size, m.occupied().tobytes(), [a.tobytes() for a in m.read(S.all_keys(name))])
    # prune = 0, occupied_only = 1 is the flat map's occupied list
    leaves, depth = m.leaves(prune=False, occupied_only=True)
    assert leaves.tobytes() == m.occupied().tobytes() and (depth == 16).all()


@pytest.mark.parametrize("name", S.NAMES)
def test_the_ot_file_parses_back_to_the_flat_map(name, twins, tmp_path):
    """the file of sindh_occmap_write_ot through a parser that shares nothing with any writer: every leaf expanded gives FlatMap.vox exactly (keys, value bits,
    colours); the header is the contract's text"""
    m = twins[name]; flat = S.reference_flat(name)[0]
    want = {k: (int(np.float32(v[0]).view(np.uint32)), v[1]) for k, v in flat.vox.items()}
    for pr, ic in S.SETTINGS:
        path = tmp_path / f"{name}_{pr}{ic}.ot"; m.write_ot(str(path), pr, ic); blob = path.read_bytes(); ref = S.reference_tree(name, pr, ic)
        assert blob == ref["ot"]
        n = ref["stats"]["n_nodes"]; res = {0.1: "0.1", 0.25: "0.25"}[flat.P.res]
        head = ("# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\nid ColorOcTree\n"
                f"size {n}\nres {res}\ndata\n").encode()
        assert blob[:len(head)] == head and len(blob) == len(head) + 8 * n
        tid, size, pres, leaves = T.parse_ot(blob)
        assert tid == "ColorOcTree" and size == n and pres == flat.P.res and len(leaves) == ref["stats"]["n_leaves"]
        assert T.expand(leaves) == want
        assert [(k, d, int(np.float32(v).view(np.uint32)), c) for k, d, v, c in T.Tree(flat, bool(pr), bool(ic)).leaf_nodes()] == leaves


def test_the_resolution_prints_as_a_default_precision_stream_prints_it(tmp_path):
    for res, text in ((0.02, "0.02"), (0.05, "0.05"), (1.0, "1"), (0.123456789, "0.123457"), (1e-5, "1e-05"), (250000.0, "250000"), (1e6, "1e+06")):
        m = OccupancyMap(res, max_voxels=16, max_points=16, host=True); path = tmp_path / "r.ot"; m.write_ot(str(path)); m.close()
        assert path.read_bytes().split(b"\n")[4:6] == [b"size 0", b"res " + text.encode()] and "%g" % res == text


def test_the_online_pruning_tree_and_the_snapshot():
    """the reference prunes ONLINE, the snapshot is the fully pruned form of the flat map.  Where no integrateNodeColor met a pruned leaf the two have the same leaves;
    where one did, they differ -- the divergence, stated as a test"""
    def online_leaves(tree):
        out = []
        def walk(n, d, k):
            if n.ch is None:
                out.append((k, d, float(n.v), n.c)); return
            s = 15 - d
            for i, c in enumerate(n.ch):
                if c is not None:
                    walk(c, d + 1, (k[0] | ((i & 1) << s), k[1] | (((i >> 1) & 1) << s), k[2] | (((i >> 2) & 1) << s)))
        walk(tree.root, 0, (0, 0, 0))
        return out
    flat, tree = S.reference_flat("shell_small", True)
    assert tree.n_pruned_colour == 0 and tree.n_prunes > 0
    snap = [(k, d, float(v), c) for k, d, v, c in T.Tree(flat, True).leaf_nodes()]
    assert online_leaves(tree) == snap and len({d for _, d, _, _ in snap}) == 3
    flat, _, tree = S0.reference("prune_block")
    assert tree.n_pruned_colour > 0
    a, b = online_leaves(tree), [(k, d, float(v), c) for k, d, v, c in T.Tree(flat, True).leaf_nodes()]
    assert a != b and len(a) == 1 and a[0][1] == 15 and a[0][3] == (12, 34, 56) and len(b) == 8      # online: one coloured depth-15 leaf; snapshot: seven white voxels and one coloured


def test_errors_and_capacity(twins):
    from sindslam_amd.cloud import _host_lib
    import ctypes as C
    L = _host_lib(); m = twins["shell_small"]; ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert TREE_STATS_DTYPE.itemsize == 22 * 4
    ref = S.reference_tree("shell_small", 1, 0); n = ref["stats"]["n_nodes"]; nl = ref["stats"]["n_leaves"]
    st = np.zeros(1, TREE_STATS_DTYPE); cnt = np.zeros(1, np.int32); data = np.full(8 * n, 7, np.uint8); leaves = np.zeros(nl, POINT_DTYPE); depth = np.full(nl, 99, np.uint8)
    assert L.sindh_occmap_tree(m._h, 1, 0, 0, None, C.c_size_t(0), None, None, 0, None, None) == SIND_E_ARG
    assert L.sindh_occmap_tree(None, 1, 0, 0, None, C.c_size_t(0), None, None, 0, None, ptr(st)) == SIND_E_ARG
    assert L.sindh_occmap_tree(m._h, 1, 0, 0, None, C.c_size_t(0), None, ptr(depth), 0, None, ptr(st)) == SIND_E_ARG
    # too small by one byte / one leaf: the counts are filled, the outputs untouched
    assert L.sindh_occmap_tree(m._h, 1, 0, 0, ptr(data), C.c_size_t(8 * n - 1), None, None, 0, ptr(cnt), ptr(st)) == SIND_E_CAPACITY
    assert st[0]["n_nodes"] == n and cnt[0] == nl and (data == 7).all()
    st[:] = 0; cnt[:] = 0
    assert L.sindh_occmap_tree(m._h, 1, 0, 0, ptr(data), C.c_size_t(8 * n), ptr(leaves), ptr(depth), nl - 1, ptr(cnt), ptr(st)) == SIND_E_CAPACITY
    assert st[0]["n_leaves"] == nl and cnt[0] == nl and (data == 7).all() and (depth == 99).all()
    # exactly enough; the depths are optional
    assert L.sindh_occmap_tree(m._h, 1, 0, 0, ptr(data), C.c_size_t(8 * n), ptr(leaves), None, nl, ptr(cnt), ptr(st)) == 0
    assert data.tobytes() == ref["data"] and leaves.tobytes() == ref["leaves"][0][0].tobytes()
    nocc = ref["stats"]["n_occupied_leaves"]; assert 0 < nocc < nl
    assert L.sindh_occmap_tree(m._h, 1, 0, 1, None, C.c_size_t(0), ptr(leaves), ptr(depth), nocc, ptr(cnt), ptr(st)) == 0 and cnt[0] == nocc
    assert leaves[:nocc].tobytes() == ref["leaves"][1][0].tobytes() and depth[:nocc].tobytes() == ref["leaves"][1][1].tobytes()
    assert L.sindh_occmap_write_ot(m._h, 1, 0, None) == SIND_E_ARG and L.sindh_occmap_write_ot(m._h, 1, 0, b"/nonexistent-directory/x.ot") == SIND_E_ARG


def _fnv(b):
    h = FNV0
    for x in bytes(b):
        h = ((h ^ x) * FNVP) & M64
    return h


def test_a_sanitizer_build_of_the_tree_twin_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_occmap_tree / sindh_occmap_write_ot with -fsanitize=address,undefined, run as a program of its own: every output array exactly as long as
    the counts say.  Nothing is loaded into python."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "occmap_tree_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "sindslam_amd", "csrc"), "sanitize-occmap-tree", "OUT=" + exe], check=True, capture_output=True, text=True)
    names = ["shell_small", "block8", "block64", "near_inner", "near_colour", "one_voxel", "empty", "white_only", "random_cloud"]
    blob = struct.pack("<i", len(names)); want = []
    for name in names:
        res, frames = S.SCENE[name]()
        blob += struct.pack("<d3i", res, S.MAX_VOXELS, S.MAX_POINTS, len(frames))
        for c, o in frames:
            blob += struct.pack("<3i", 1, len(c), 0) + struct.pack("<i", len(c)) + np.array(o, np.float32).tobytes() + np.ascontiguousarray(c).tobytes()
        for flags in range(8):
            pr, ic, occ = flags & 1, (flags >> 1) & 1, (flags >> 2) & 1; ref = S.reference_tree(name, pr, ic); st = ref["stats"]; pts, depth = ref["leaves"][occ]
            want.append(" ".join(str(v) for v in [st["n_nodes"], st["n_inner"], st["n_leaves"], st["n_pruned"], st["n_occupied_leaves"]] + st["leaves_at_depth"]
                                 + [len(pts), _fnv(ref["data"]), _fnv(pts.tobytes()), _fnv(depth.tobytes())]))
        want.append(str(len(S.reference_tree(name, 1, 0)["ot"])))
    path = tmp_path / "records.bin"; path.write_bytes(blob)
    r = subprocess.run([exe, str(path), str(tmp_path / "out.ot")], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stdout.splitlines() == want
