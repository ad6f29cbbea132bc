"""Timing of sind_match_sim3_optimize, the recipe of profiles/match_sim3_opt.txt: B = 1 and B = 3 (a typical number of consistent loop candidates) with n = 64 and n = 256 pairs, 30 %
outliers, 0.5 px noise, fix_scale as the RGB-D system runs; the device call against the host library's sindh_sim3_optimize on the same items, alternating, 200 timed repetitions after 10.
A host clock around each call: the device call ends in a stream synchronise; the Python wrapper's array preparation is inside both clocks."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import poseopt_scene as P, sim3_scene as S3, sim3opt_scene as SC
from sindslam_amd.matcher import ORBmatcher

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
mt = ORBmatcher(*[float(k) for k in P.K5], (0, 640, 0, 480), S3.scale_factors(), cap=4096, max_batch=3)
host = SC.HostOptimizer()
for B in (1, 3):
    for n in (64, 256):
        items = [SC.scene(900 + 10 * n + b, n, outliers=0.3, noise=0.5) for b in range(B)]
        dev, cpu = mt.OptimizeSim3(items), host.OptimizeSim3(items)
        equal = all(np.array_equal(SC.bits(np.asarray(d[k])), SC.bits(np.asarray(c[k]))) for d, c in zip(dev, cpu) for k in SC.OUTPUTS)
        for _ in range(10):
            mt.OptimizeSim3(items); host.OptimizeSim3(items)
        td, th = [], []
        for _ in range(reps):                                            # alternating, so that what else the machine does falls on both
            a = time.perf_counter(); mt.OptimizeSim3(items); b = time.perf_counter(); host.OptimizeSim3(items); c = time.perf_counter()
            td.append((b - a) * 1e3); th.append((c - b) * 1e3)
        pct = lambda t: [round(float(np.percentile(t, q)), 4) for q in (50, 10, 90)]
        print(f"B={B} n={n}", json.dumps(dict(equal=equal, iterations=[int(d["stage_iters"].sum()) for d in dev], device_ms_p50_p10_p90=pct(td), host_ms_p50_p10_p90=pct(th))), flush=True)
mt.close()
