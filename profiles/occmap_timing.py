"""Timing of sind_occmap_*, the recipe of profiles/occmap.txt.  Resolution 0.02, the reference's probabilities.  Cases: the stream key frame t = 8 alone (B = 1), the
key frames t = 8 and t = 12 in one call (B = 2), both read where sind_cloud_generate left them (insertGenerated: nothing uploaded); a full 76 800-point cloud (every
stride-2 pixel of the t = 8 depth frame back-projected, uploaded by the call); each into a CLEARED map (the clear is outside the clock), the device against the host twin on
one core, ALTERNATING.  Then occupied() against the map size.  A host clock around each call; the device insert ends in its one stream wait.  No parent code exists to
compare with, and octomap itself was never timed: it is not available here.
    python profiles/occmap_timing.py [reps]          timed device repetitions (default 10); the twin runs in the first max(reps // 5, 2) of them
    python profiles/occmap_timing.py tree RES        no device: the pruning tree of tests/occmap_ref.py (pure Python) on the key frame t = 8 at resolution RES: how many
                                                     integrateNodeColor calls met a pruned leaf (the contract's second divergence)
Per launch: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/occmap_timing.py 3"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloud_scene as CS
import occmap_scene as S
from sindslam_amd.synth import SyntheticStream

KEYS = ("imgRGB", "imgDepth", "imgDepthLast", "imgDynaMask", "imgDynaMaskLast", "imgLabel", "poseRelative", "Twc")
stream = SyntheticStream()
scenes = [CS.keyframe_pair(stream, t, gap) for t, gap in ((8, 2), (12, 1))]
cam5 = scenes[0][0]

if len(sys.argv) > 2 and sys.argv[1] == "tree":
    import occmap_ref as R
    import oracle_lib as O
    res = float(sys.argv[2]); a = scenes[0][1]
    cloud = O.generate_point_cloud(cam5, *[a[k] for k in KEYS])["points"]; origin = tuple(a["Twc"][:3, 3].astype(np.float32))
    P = R.Params(res); flat = R.FlatMap(P); tree = R.PruneTree(P); t0 = time.perf_counter()
    st = flat.insert(cloud, origin, tree)
    differ = sum(tree.search(k)[0].c != v[1] for k, v in flat.vox.items())
    print("pruning tree, key frame t = 8", json.dumps(dict(resolution=res, points=len(cloud), stats=st, known_voxels=len(flat.vox), prunes=tree.n_prunes,
                                                           colour_integrations_on_a_pruned_leaf=tree.n_pruned_colour, voxels_whose_colour_differs=int(differ),
                                                           logodds_equal=all(tree.search(k)[0].v == v[0] for k, v in flat.vox.items()), seconds=round(time.perf_counter() - t0, 1))))
    sys.exit(0)

from sindslam_amd.cloud import CloudGenerator
from sindslam_amd.occupancy import OccupancyMap

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
MAXV = 1 << 22; SLOTS = 2 * MAXV
gen = CloudGenerator(*cam5, max_batch=2)
args2 = [np.stack([s[1][k] for s in scenes]) for k in KEYS]; Twc = args2[-1]
kf = [r["points"] for r in gen.generatePointCloud(*args2)]; org = Twc[:, :3, 3].astype(np.float32)
depth = scenes[0][1]["imgDepth"][::2, ::2].astype(np.float32) / np.float32(cam5[4]); depth[(depth < 0.3) | (depth > 9)] = 3.0
v, u = np.mgrid[0:480:2, 0:640:2].astype(np.float32)
full = S.cloud(np.stack([(u - cam5[2]) * depth / cam5[0], (v - cam5[3]) * depth / cam5[1], depth], -1))
dev = OccupancyMap(0.02, max_voxels=MAXV, max_points=76800); host = OccupancyMap(0.02, max_voxels=MAXV, max_points=76800, host=True)
cases = [("key frame t = 8, B = 1 (insertGenerated)", lambda: dev.insertGenerated(gen, Twc[:1]), lambda: host.insert(kf[:1], org[:1])),
         ("key frames t = 8 and t = 12, B = 2 (insertGenerated)", lambda: dev.insertGenerated(gen, Twc), lambda: host.insert(kf, org)),
         ("full cloud, 76 800 points (uploaded)", lambda: dev.insert([full], [(0.0, 0.0, 0.0)]), lambda: host.insert([full], [(0.0, 0.0, 0.0)]))]
pct = lambda t: [round(float(np.percentile(t, q)), 3) for q in (50, 10, 90)]
for name, fd, fh in cases:
    dev.clear(); host.clear(); sd = fd(); sh = fh()
    od, oh = dev.occupied(), host.occupied()
    equal = [tuple(int(x) for x in a) for a in sd] == [tuple(int(x) for x in a) for a in sh] and dev.size == host.size and od.tobytes() == oh.tobytes()
    share = dict(rays=[int(s["n_rays"]) for s in sd], voxel_updates=[int(s["n_rays"] + s["n_miss_updates"]) for s in sd], new_voxels=[int(s["n_new_voxels"]) for s in sd],
                 known=dev.size, table_load=round(dev.size / SLOTS, 4), occupied=len(od))
    for _ in range(2):
        dev.clear(); fd()
    td, th, to, toh = [], [], [], []
    for r in range(reps):
        dev.clear(); a = time.perf_counter(); fd(); b = time.perf_counter(); td.append((b - a) * 1e3)
        a = time.perf_counter(); dev.occupied(); b = time.perf_counter(); to.append((b - a) * 1e3)
        if r < max(reps // 5, 2):
            host.clear(); a = time.perf_counter(); fh(); b = time.perf_counter(); host.occupied(); c = time.perf_counter(); th.append((b - a) * 1e3); toh.append((c - b) * 1e3)
    print(name, json.dumps(dict(equal=bool(equal), device_ms_p50_p10_p90=pct(td), host_twin_ms_p50_p10_p90=pct(th), occupied_device_ms=pct(to), occupied_twin_ms=pct(toh), **share)), flush=True)
gen.close(); dev.close(); host.close()
