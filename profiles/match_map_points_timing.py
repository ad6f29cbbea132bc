"""Timing of sind_match_triangulate and sind_match_update_points, the recipe of profiles/match_map_points.txt: Triangulate on 10 pairs x 150 matches (CreateNewMapPoints of
one key frame), UpdateMapPoints on 1 000 points x 8 observations (after Fuse), 2 000 x 5 (after local BA) and 20 000 x 6 (after a loop closure), both updates; the device
call against the host library's twin on the same items, alternating, `reps` timed repetitions after 3.  A host clock around each call: the device call ends in a stream
synchronise; the Python wrapper's array preparation is inside both clocks."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import mappoints_scene as SC
from sindslam_amd.matcher import ORBmatcher

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
mt = ORBmatcher(*[float(k) for k in SC.K5], (0, 640, 0, 480), SC.SCALE, cap=512, max_batch=10)
host = SC.HostMap()
pairs = [SC.tri_scene(900 + b, 150, "mixed", unmatched=0, wrong=0.05) for b in range(10)]
cases = [("Triangulate 10 x 150", "Triangulate", pairs, SC.TRI_OUT)]
for name, n, c in (("after Fuse", 1000, 8), ("after local BA", 2000, 5), ("after a loop closure", 20000, 6)):
    cases.append((f"UpdateMapPoints {n} x {c} ({name})", "UpdateMapPoints", [SC.mp_scene(910 + c, [c] * n, n_kf=64)], SC.MP_OUT))
for name, call, items, outs in cases:
    dev, cpu = getattr(mt, call)(items), getattr(host, call)(items)
    equal = all(np.array_equal(SC.LS.bits(np.asarray(d[k])), SC.LS.bits(np.asarray(c[k]).astype(np.asarray(d[k]).dtype))) for d, c in zip(dev, cpu) for k in outs)
    for _ in range(3):
        getattr(mt, call)(items); getattr(host, call)(items)
    td, th = [], []
    for _ in range(reps):                                                # alternating, so that what else the machine does falls on both
        a = time.perf_counter(); getattr(mt, call)(items); b = time.perf_counter(); getattr(host, call)(items); c = time.perf_counter()
        td.append((b - a) * 1e3); th.append((c - b) * 1e3)
    pct = lambda t: [round(float(np.percentile(t, q)), 3) for q in (50, 10, 90)]
    print(name, json.dumps(dict(equal=equal, device_ms_p50_p10_p90=pct(td), host_ms_p50_p10_p90=pct(th))), flush=True)
mt.close()
