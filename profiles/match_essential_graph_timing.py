"""Timing of sind_match_essential_graph, the recipe of profiles/match_essential_graph.txt: B = 1 and B = 4 at 50 and 250 key frames (tests/essgraph_scene.scene: the
drifted circle, a spanning tree, covisibility window 10, a loop between the last 5 and the first 5 key frames with their CorrectedSim3 / NonCorrectedSim3 entries),
20 000 map points per item, fix_scale; the device call against the host library's sindh_essential_graph on the same items, alternating, `reps` timed repetitions after
3.  A host clock around each call: the device call ends in a stream synchronise; the Python wrapper's array preparation and the digest of the items into the kernel's
lists are inside both clocks."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import essgraph_scene as SC
from sindslam_amd.matcher import ORBmatcher

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [50, 250]
mt = ORBmatcher(520.0, 516.0, 320.0, 240.0, 40.0, (0, 640, 0, 480), [1.2 ** k for k in range(8)], cap=192, max_batch=4)
host = SC.HostEss()
for B in (1, 4):
    for n_kf in sizes:
        items = [SC.scene(700 + n_kf + b, n_kf, window=10, loop=5, n_mp=20000, drift=(0.004 * 12 / n_kf, 0.02 * 12 / n_kf)) for b in range(B)]
        dev, cpu = mt.OptimizeEssentialGraph(items, True), host.OptimizeEssentialGraph(items, True)
        equal = all(np.array_equal(SC.bits(np.asarray(d[k])), SC.bits(np.asarray(c[k]))) for d, c in zip(dev, cpu) for k in SC.OUTPUTS)
        env = [SC.linear(dict(i, x3Dw=np.zeros((0, 3), np.float32), mp_ref=np.zeros(0, np.int32)))[5] for i in items[:1]]
        for _ in range(3):
            mt.OptimizeEssentialGraph(items, True); host.OptimizeEssentialGraph(items, True)
        td, th = [], []
        for _ in range(reps):                                            # alternating, so that what else the machine does falls on both
            a = time.perf_counter(); mt.OptimizeEssentialGraph(items, True); b = time.perf_counter(); host.OptimizeEssentialGraph(items, True); c = time.perf_counter()
            td.append((b - a) * 1e3); th.append((c - b) * 1e3)
        pct = lambda t: [round(float(np.percentile(t, q)), 3) for q in (50, 10, 90)]
        print(f"B={B} key frames={n_kf}", json.dumps(dict(equal=equal, edges=[len(i["edge_i"]) for i in items], unknowns=[7 * d["n_active"] for d in dev], envelope_entries=env,
                                                         iterations=[d["n_iters"] for d in dev], solver_fail=[d["solver_fail"] for d in dev], chi2=[float(d["chi2"]) for d in dev],
                                                         device_ms_p50_p10_p90=pct(td), host_ms_p50_p10_p90=pct(th))), flush=True)
mt.close()
