"""Timing of sind_match_local_ba, the recipe of profiles/match_local_ba.txt: B = 1 and B = 4 with a small window (5 local key frames + 5 fixed cameras, 300 points, every
point seen by 5 of the 10) and a typical one (20 + 20 key frames, 2 000 points, 5 observations each: 10 000 observations), mixed monocular / stereo, 0.5 px noise, 2 % planted
outliers; the device call against the host library's sindh_local_ba on the same items, alternating, `reps` timed repetitions after 3.  A host clock around each call: the
device call ends in a stream synchronise; the Python wrapper's array preparation and the digest of the items into the kernel's lists are inside both clocks."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import localba_scene as SC, sim3_scene as S3
from sindslam_amd.matcher import ORBmatcher

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
mt = ORBmatcher(*[float(k) for k in SC.K5], (0, 640, 0, 480), S3.scale_factors(), cap=192, max_batch=4)
host = SC.HostBA()
for B in (1, 4):
    for name, (n_local, n_fixed, n_pts) in (("small", (5, 5, 300)), ("typical", (20, 20, 2000))):
        items = [SC.scene(900 + n_pts + b, n_local, n_fixed, n_pts, kind="mixed", outliers=n_pts // 10, obs_per_point=5) for b in range(B)]
        dev, cpu = mt.LocalBundleAdjustment(items), host.LocalBundleAdjustment(items)
        equal = all(np.array_equal(SC.bits(np.asarray(d[k])), SC.bits(np.asarray(c[k]))) for d, c in zip(dev, cpu) for k in SC.OUTPUTS)
        for _ in range(3):
            mt.LocalBundleAdjustment(items); host.LocalBundleAdjustment(items)
        td, th = [], []
        for _ in range(reps):                                            # alternating, so that what else the machine does falls on both
            a = time.perf_counter(); mt.LocalBundleAdjustment(items); b = time.perf_counter(); host.LocalBundleAdjustment(items); c = time.perf_counter()
            td.append((b - a) * 1e3); th.append((c - b) * 1e3)
        pct = lambda t: [round(float(np.percentile(t, q)), 3) for q in (50, 10, 90)]
        print(f"B={B} {name}", json.dumps(dict(equal=equal, observations=[len(i["obs_kf"]) for i in items], iterations=[[int(v) for v in d["stage_iters"]] for d in dev],
                                               device_ms_p50_p10_p90=pct(td), host_ms_p50_p10_p90=pct(th))), flush=True)
mt.close()
