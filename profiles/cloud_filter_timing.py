"""Timing of sind_cloud_filter_outliers, the recipe of profiles/cloud_filter.txt: mean_k = 100, stddev_mul = 1.0 on one and four stream key-frame clouds, a full 76 800-point
cloud (every stride-2 pixel of a 640 x 480 stream depth frame valid) and the far-cluster scene of the tests; the device (points uploaded by the call) against the host twin
on one core and against scipy's cKDTree (build + query of k = 101 over the finite points, one worker: the only independent k-d tree here; it does the search alone, not the
sums), ALTERNATING; and generatePointCloud with and without filter= (the points == NULL path: nothing uploaded but the images).  A host clock around each call; the device call
ends in its second stream wait; the Python wrapper's packing (the same code for device and twin) is inside both clocks.  argv[1] = timed device repetitions (default 20);
the twin and the tree run in the first max(reps // 5, 3) of them."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloud_filter_scene as S
import cloud_scene as CS
from scipy.spatial import cKDTree
from sindslam_amd.cloud import CloudGenerator, POINT_DTYPE, filterOutliersHost
from sindslam_amd.synth import SyntheticStream

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
KEYS = ("imgRGB", "imgDepth", "imgDepthLast", "imgDynaMask", "imgDynaMaskLast", "imgLabel", "poseRelative", "Twc")
stream = SyntheticStream()
scenes = [CS.keyframe_pair(stream, t, gap) for t, gap in ((8, 2), (12, 1))]
cam5 = scenes[0][0]
gen = CloudGenerator(*cam5, max_batch=4)
args2 = [np.stack([s[1][k] for s in scenes]) for k in KEYS]
kf = [r["points"] for r in gen.generatePointCloud(*args2)]
depth = scenes[0][1]["imgDepth"][::2, ::2].astype(np.float32) / np.float32(cam5[4]); depth[(depth < 0.3) | (depth > 9)] = 3.0
v, u = np.mgrid[0:480:2, 0:640:2].astype(np.float32)
full = S.cloud(np.stack([(u - cam5[2]) * depth / cam5[0], (v - cam5[3]) * depth / cam5[1], depth], -1))
cases = [("1 key-frame cloud", [kf[0]]), ("4 key-frame clouds", [kf[0], kf[1], kf[0], kf[1]]), ("full cloud, 76 800 points", [full]), ("far-cluster scene, 4 061 points", [S.random_far()])]


def tree(clouds):
    out = []
    for p in clouds:
        xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64); xyz = xyz[np.isfinite(xyz).all(1)]
        d, _ = cKDTree(xyz).query(xyz, k=101); out.append(d[:, 1:].mean(1))
    return out


pct = lambda t: [round(float(np.percentile(t, q)), 3) for q in (50, 10, 90)]
for name, clouds in cases:
    d = gen.filterOutliers(clouds, 100, 1.0); h = filterOutliersHost(clouds, 100, 1.0)
    equal = all(np.array_equal(a["distances"].view(np.uint32), b["distances"].view(np.uint32)) and a["points"].tobytes() == b["points"].tobytes() and a["stats"].tobytes()[:32] == b["stats"].tobytes()[:32]
                for a, b in zip(d, h))
    share = dict(points=[len(c) for c in clouds], finite=[a["valid"] for a in d], kept=[len(a["points"]) for a in d], ring=[a["n_ring"] for a in d], brute=[a["n_brute"] for a in d])
    for _ in range(3):
        gen.filterOutliers(clouds, 100, 1.0)
    td, th, tt = [], [], []
    for r in range(reps):                                                # alternating, so that what else the machine does falls on all three
        a = time.perf_counter(); gen.filterOutliers(clouds, 100, 1.0); b = time.perf_counter(); td.append((b - a) * 1e3)
        if r < max(reps // 5, 3):
            filterOutliersHost(clouds, 100, 1.0); c = time.perf_counter(); tree(clouds); e = time.perf_counter()
            th.append((c - b) * 1e3); tt.append((e - c) * 1e3)
    print(name, json.dumps(dict(equal=bool(equal), device_ms_p50_p10_p90=pct(td), host_twin_ms_p50_p10_p90=pct(th), ckdtree_ms_p50_p10_p90=pct(tt), **share)), flush=True)

for _ in range(3):
    gen.generatePointCloud(*args2); gen.generatePointCloud(*args2, filter=True)
tg, tf = [], []
for r in range(reps):
    a = time.perf_counter(); gen.generatePointCloud(*args2); b = time.perf_counter(); gen.generatePointCloud(*args2, filter=True); c = time.perf_counter()
    tg.append((b - a) * 1e3); tf.append((c - b) * 1e3)
print("generatePointCloud, 2 key frames", json.dumps(dict(generate_ms_p50_p10_p90=pct(tg), generate_and_filter_ms_p50_p10_p90=pct(tf))), flush=True)
gen.close()
