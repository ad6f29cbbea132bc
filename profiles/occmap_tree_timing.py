"""Timing of sind_occmap_tree, the recipe of profiles/occmap_tree.txt (the maps are those of profiles/occmap.txt).  Resolution 0.02, the reference's probabilities.
Maps: after the stream key frame t = 8; after t = 8 and t = 12; after a full 76 800-point cloud (every stride-2 pixel of the t = 8 depth frame back-projected).  Per map,
on the C ABI with output arrays of exactly the reported sizes (the Python wrapper would call twice: the counts, then the outputs):
  tree        prune = 1, inner_colour = 0, the stream and all leaves: the device against the host twin on one core, ALTERNATING
  counts      the same with NULL outputs (the bottom-up half and one wait), device only
  occupied    prune = 0, occupied_only = 1, leaves only, against sind_occmap_occupied (which sorts on the host), device only
2 untimed calls, then `reps` timed ones; a host clock around each call; every device call ends in its last stream wait.
    python profiles/occmap_tree_timing.py [reps]          (default 10)
Per kernel, in a run of its own: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/occmap_tree_timing.py 3"""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloud_scene as CS
import occmap_scene as S
from sindslam_amd._lib import lib, ptr
from sindslam_amd.cloud import POINT_DTYPE, CloudGenerator, _host_lib
from sindslam_amd.occupancy import TREE_STATS_DTYPE, OccupancyMap
from sindslam_amd.synth import SyntheticStream

KEYS = ("imgRGB", "imgDepth", "imgDepthLast", "imgDynaMask", "imgDynaMaskLast", "imgLabel", "poseRelative", "Twc")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
stream = SyntheticStream()
scenes = [CS.keyframe_pair(stream, t, gap) for t, gap in ((8, 2), (12, 1))]
cam5 = scenes[0][0]; MAXV = 1 << 22
gen = CloudGenerator(*cam5, max_batch=2)
args2 = [np.stack([s[1][k] for s in scenes]) for k in KEYS]; Twc = args2[-1]
kf = [r["points"] for r in gen.generatePointCloud(*args2)]; org = Twc[:, :3, 3].astype(np.float32)
depth = scenes[0][1]["imgDepth"][::2, ::2].astype(np.float32) / np.float32(cam5[4]); depth[(depth < 0.3) | (depth > 9)] = 3.0
v, u = np.mgrid[0:480:2, 0:640:2].astype(np.float32)
full = S.cloud(np.stack([(u - cam5[2]) * depth / cam5[0], (v - cam5[3]) * depth / cam5[1], depth], -1))
dev = OccupancyMap(0.02, max_voxels=MAXV, max_points=76800); host = OccupancyMap(0.02, max_voxels=MAXV, max_points=76800, host=True)
cases = [("map after key frame t = 8", kf[:1], org[:1]), ("map after key frames t = 8 and t = 12", kf, org), ("map after the full cloud, 76 800 points", [full], [(0.0, 0.0, 0.0)])]
pct = lambda t: [round(float(np.percentile(t, q)), 3) for q in (50, 10, 90)]
LD, LH = lib(), _host_lib()


def call(f, m, prune, colour, occ, data, leaves, depths):
    st = np.zeros(1, TREE_STATS_DTYPE); n = np.zeros(1, np.int32)
    rc = f(m._h, prune, colour, occ, ptr(data) if data is not None and len(data) else None, C.c_size_t(0 if data is None else len(data)),
           ptr(leaves) if leaves is not None and len(leaves) else None, ptr(depths) if depths is not None and len(depths) else None, 0 if leaves is None else len(leaves), ptr(n), ptr(st))
    assert rc == 0, rc
    return st[0], int(n[0])


def clock(fn):
    a = time.perf_counter(); fn(); return (time.perf_counter() - a) * 1e3


for name, clouds, origins in cases:
    dev.clear(); host.clear(); dev.insert(clouds, origins); host.insert(clouds, origins)
    flat, _ = call(LD.sind_occmap_tree, dev, 0, 0, 0, None, None, None); st, nl = call(LD.sind_occmap_tree, dev, 1, 0, 0, None, None, None)
    bufs = lambda n_nodes, n_leaves: (np.zeros(8 * n_nodes, np.uint8), np.zeros(n_leaves, POINT_DTYPE), np.zeros(n_leaves, np.uint8))
    dd, dl, dp = bufs(int(st["n_nodes"]), nl); hd, hl, hp = bufs(int(st["n_nodes"]), nl)
    nocc = len(dev.occupied()); ol, op = np.zeros(nocc, POINT_DTYPE), np.zeros(nocc, np.uint8); oo = np.zeros(max(nocc, 1), POINT_DTYPE); on = np.zeros(1, np.int32)
    f_tree = lambda: call(LD.sind_occmap_tree, dev, 1, 0, 0, dd, dl, dp); f_twin = lambda: call(LH.sindh_occmap_tree, host, 1, 0, 0, hd, hl, hp)
    f_counts = lambda: call(LD.sind_occmap_tree, dev, 1, 0, 0, None, None, None); f_occ = lambda: call(LD.sind_occmap_tree, dev, 0, 0, 1, None, ol, op)
    f_flat = lambda: LD.sind_occmap_occupied(dev._h, ptr(oo), len(oo), ptr(on))
    for _ in range(2):
        f_tree(); f_counts(); f_occ(); f_flat()
    f_twin()
    t = dict(tree=[], twin=[], counts=[], occ=[], flat=[])
    for r in range(reps):
        t["tree"].append(clock(f_tree)); t["twin"].append(clock(f_twin)); t["counts"].append(clock(f_counts)); t["occ"].append(clock(f_occ)); t["flat"].append(clock(f_flat))
    equal = dd.tobytes() == hd.tobytes() and dl.tobytes() == hl.tobytes() and dp.tobytes() == hp.tobytes() and ol.tobytes() == oo[:nocc].tobytes() and on[0] == nocc
    print(name, json.dumps(dict(equal=bool(equal), known=dev.size, nodes_unpruned=int(flat["n_nodes"]), inner_unpruned=int(flat["n_inner"]), nodes_pruned=int(st["n_nodes"]),
                                inner_pruned=int(st["n_inner"]), n_pruned=int(st["n_pruned"]), occupied_leaves_pruned=int(st["n_occupied_leaves"]), occupied_voxels=nocc,
                                leaves_at_depth={d: int(c) for d, c in enumerate(st["leaves_at_depth"]) if c}, stream_bytes=len(dd),
                                tree_device_ms_p50_p10_p90=pct(t["tree"]), tree_twin_ms_p50_p10_p90=pct(t["twin"]), counts_device_ms=pct(t["counts"]),
                                occupied_leaves_tree_ms=pct(t["occ"]), occupied_flat_ms=pct(t["flat"]))), flush=True)
gen.close(); dev.close(); host.close()
