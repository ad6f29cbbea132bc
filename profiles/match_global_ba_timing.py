"""Timing of sind_match_global_ba, the recipe of profiles/match_global_ba.txt.  Cases: the "typical" window of profiles/match_local_ba.txt converted (20 free key
frames and the fixed one, 2 000 points, 5 observations each: 10 000 observations, mixed monocular / stereo) and a loop-closure map at the sizes of
profiles/match_essential_graph.txt (50 and 250 key frames, 20 000 points, 5 observations each inside a window of 10 key frames, one loop), at iterations = 10 without
kernels, as LoopClosing::RunGlobalBundleAdjustment calls it.  The device call against the host library's sindh_global_ba on one core, alternating, `reps` timed
repetitions after 2, bit patterns compared first.  On the all-stereo variant of the first case, the parent's sind_match_local_ba(do_more = 0) against the new call at
iterations = 5 with kernels: the same arithmetic (compared as bits), one workgroup against the grid.  A host clock around each call: the device calls end in a stream
synchronise; the Python wrapper's array preparation and the digest of the item into the kernels' lists are inside every clock."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import globalba_scene as G, localba_scene as SC, sim3_scene as S3
from sindslam_amd.matcher import ORBmatcher

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
mt = ORBmatcher(*[float(k) for k in SC.K5], (0, 640, 0, 480), S3.scale_factors(), cap=192, max_batch=1)
host = G.HostGBA()
pct = lambda t: [round(float(np.percentile(t, q)), 3) for q in (50, 10, 90)]


def clock(f, g):
    for _ in range(2):
        f(); g()
    tf, tg = [], []
    for _ in range(reps):                                                # alternating, so that what else the machine does falls on both
        a = time.perf_counter(); f(); b = time.perf_counter(); g(); c = time.perf_counter()
        tf.append((b - a) * 1e3); tg.append((c - b) * 1e3)
    return pct(tf), pct(tg)


cases = [("typical window, 21 key frames", G.band_map(2900, 21, 2000, 21, 5, kind="mixed", outliers=200)),
         ("loop map, 50 key frames", G.band_map(2950, 50, 20000, 10, 5, loops=((2, 47),), kind="mixed", outliers=400)),
         ("loop map, 250 key frames", G.band_map(3150, 250, 20000, 10, 5, loops=((2, 247),), kind="mixed", outliers=400))]
for name, it in cases:
    dev, cpu = mt.GlobalBundleAdjustment([it], 10, False)[0], host.GlobalBundleAdjustment([it], 10, False)[0]
    equal = all(np.array_equal(SC.bits(np.asarray(dev[k])), SC.bits(np.asarray(cpu[k]))) for k in G.OUTPUTS)
    launches, waits = mt.global_ba_counts()
    td, th = clock(lambda: mt.GlobalBundleAdjustment([it], 10, False), lambda: host.GlobalBundleAdjustment([it], 10, False))
    print(name, json.dumps(dict(equal=equal, observations=len(it["obs_kf"]), iterations=dev["n_iters"], active_poses=dev["n_active_poses"], launches=launches, host_waits=waits,
                                env_entries=dev["env_entries"], env_dense_entries=dev["env_dense_entries"], device_ms_p50_p10_p90=td, host_ms_p50_p10_p90=th)), flush=True)

s = dict(SC.scene(2900, 20, 0, 2000, kind="stereo", outliers=200, obs_per_point=5), do_more=False)
it, order = G.from_local(s)
loc, dev = mt.LocalBundleAdjustment([s])[0], mt.GlobalBundleAdjustment([it], 5, True)[0]
equal = np.array_equal(SC.bits(dev["Tcw"]), SC.bits(loc["Tcw"][order])) and np.array_equal(SC.bits(dev["x3Dw"]), SC.bits(loc["x3Dw"]))
launches, waits = mt.global_ba_counts()
tl, tg = clock(lambda: mt.LocalBundleAdjustment([s]), lambda: mt.GlobalBundleAdjustment([it], 5, True))
print("typical window all stereo, stage 1", json.dumps(dict(equal=equal, observations=len(it["obs_kf"]), iterations=dev["n_iters"], launches=launches, host_waits=waits,
                                                            local_ba_one_workgroup_ms_p50_p10_p90=tl, global_ba_grid_ms_p50_p10_p90=tg)), flush=True)
mt.close()
