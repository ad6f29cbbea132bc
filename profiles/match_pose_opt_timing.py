"""Timing of sind_match_pose_optimize, the recipe of profiles/match_pose_opt.txt: B = 1 with n = 192 and n = 4096 (the handle's default capacity) and B = max_batch = 20 with n = 192, mixed
mono / stereo, 30 % outliers, 0.5 px noise; the device call against the host library's sindh_pose_optimize on the same items, alternating, 200 timed repetitions after 10.  A host clock
around each call: the device call ends in a stream synchronise; the Python wrapper's array preparation is inside both clocks."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import poseopt_scene as P, sim3_scene as S3
from sindslam_amd.matcher import ORBmatcher

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
mt = ORBmatcher(*[float(k) for k in P.K5], (0, 640, 0, 480), S3.scale_factors(), cap=4096, max_batch=20)
host = P.HostOptimizer()
for name, items in (("B=1 n=192", [P.scene(900, 192)]), ("B=1 n=4096", [P.scene(901, 4096)]), ("B=20 n=192", [P.scene(910 + b, 192) for b in range(20)])):
    dev, cpu = mt.PoseOptimization(items), host.PoseOptimization(items)
    equal = all(np.array_equal(P.bits(d[k]), P.bits(c[k])) for d, c in zip(dev, cpu) for k in ("Tcw", "outlier", "round_pose", "round_chi2", "round_lambda"))
    for _ in range(10):
        mt.PoseOptimization(items); host.PoseOptimization(items)
    td, th = [], []
    for _ in range(reps):                                                # alternating, so that what else the machine does falls on both
        a = time.perf_counter(); mt.PoseOptimization(items); b = time.perf_counter(); host.PoseOptimization(items); c = time.perf_counter()
        td.append((b - a) * 1e3); th.append((c - b) * 1e3)
    pct = lambda t: [round(float(np.percentile(t, q)), 4) for q in (50, 10, 90)]
    print(name, json.dumps(dict(equal=equal, iterations=[int(d["round_iters"].sum()) for d in dev][:3], device_ms_p50_p10_p90=pct(td), host_ms_p50_p10_p90=pct(th))), flush=True)
mt.close()
