"""Timing of sind_covis_count and sind_covis_cull, the recipe of profiles/match_covis.txt: a map of 250 key frames x 2 000 features (1 500 of them hold a point; a key frame
sees the points of a window that moves by 200 ids per key frame, so a point has about 7 observations and a key frame shares points with about 28 others); the count for one key frame
(Q = 1) and for 40 in one call, the tracker's vote with 1 000 points, the cull of 40 key frames: the device against the host twin on one core and against the walk over the dicts
(optimizer.update_connections for the counts, the same loops written out for the vote and the cull), alternating, `reps` timed repetitions after 3.  A host clock around each call: the
device call ends in a stream synchronise; the Python wrapper's array preparation is inside the device's and the twin's clocks."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import covis_scene as SC
from sindslam_amd import covisibility as CV
from sindslam_amd import optimizer as O

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
N_KF, CAP_FEAT, SEEN, STEP, WINDOW, NLEVELS = 250, 2000, 1500, 200, 3000, 8
CAP_POINTS = N_KF * STEP + WINDOW
rng = np.random.RandomState(1)
keyframes, mappoints, ops = {}, {m: dict(obs={}, bad=False) for m in range(CAP_POINTS)}, []
for k in range(N_KF):
    pts = k * STEP + rng.permutation(WINDOW)[:SEEN]; idx = rng.permutation(CAP_FEAT)[:SEEN]
    mp = np.full(CAP_FEAT, -1, np.int64); mp[idx] = pts
    stereo = rng.rand(CAP_FEAT) < 0.67
    keyframes[k] = dict(mp=mp, octave=rng.randint(0, NLEVELS, CAP_FEAT).astype(np.int32), u_right=np.where(stereo, 100.0, -1.0).astype(np.float32),
                        depth=np.where(stereo, rng.uniform(0.5, 8, CAP_FEAT), -1).astype(np.float32), bad=False, weights={}, covisible=[])
    for i, m in zip(idx.tolist(), pts.tolist()):
        mappoints[m]["obs"][k] = i; ops.append((k, i, m, int(keyframes[k]["octave"][i]), int(stereo[i])))
dev = CV.CovisibilityTable(N_KF, CAP_FEAT, CAP_POINTS, NLEVELS, host=False, max_queries=64)
twin = CV.CovisibilityTable(N_KF, CAP_FEAT, CAP_POINTS, NLEVELS, host=True)
t0 = time.perf_counter(); SC.load(dev, ops); t1 = time.perf_counter(); SC.load(twin, ops); t2 = time.perf_counter()
print("load of", len(ops), "ops in one apply (ctypes array built inside the clock):", json.dumps(dict(device_ms=round((t1 - t0) * 1e3, 1), host_ms=round((t2 - t1) * 1e3, 1))), flush=True)
print("observations per point:", round(float(np.mean([len(p["obs"]) for p in mappoints.values() if p["obs"]])), 2), flush=True)

some = list(range(100, 140)); lists = {k: CV.good_points(keyframes[k]["mp"], mappoints) for k in some}
frame = np.concatenate([keyframes[120]["mp"][keyframes[120]["mp"] >= 0][:700], keyframes[121]["mp"][keyframes[121]["mp"] >= 0][:300]]).astype(np.int32)
cull_items = [CV.cull_item(k, keyframes, mappoints, 4.0) for k in some]


def walk_counts(ks):
    for k in ks:
        O.update_connections(k, keyframes, mappoints)
    return [np.array([keyframes[k]["weights"].get(q, 0) for q in range(N_KF)], np.int32) for k in ks]


def walk_vote():
    counter = {}
    for m in frame.tolist():
        if m >= 0 and not mappoints[m].get("bad"):
            for k in dict(mappoints[m]["obs"]):
                counter[k] = counter.get(k, 0) + 1
    return [np.array([counter.get(q, 0) for q in range(N_KF)], np.int32)]


def walk_cull():
    out = []
    for k, pts, octv, close in cull_items:
        n_mps = n_red = 0
        for i, m in enumerate(pts.tolist()):
            if m < 0 or not close[i]:
                continue
            n_mps += 1
            obs = dict(mappoints[m]["obs"])
            if sum(2 if keyframes[q]["u_right"][j] >= 0 else 1 for q, j in obs.items()) > 3:
                n = 0
                for q, j in obs.items():
                    if q != k and keyframes[q]["octave"][j] <= octv[i] + 1:
                        n += 1
                        if n >= 3:
                            break
                n_red += n >= 3
        out.append((n_mps, n_red))
    return out


cases = [("count, Q = 1", lambda t: t.count([lists[120]], [120]), lambda: walk_counts([120])),
         ("count, Q = 40", lambda t: t.count([lists[k] for k in some], some), lambda: walk_counts(some)),
         ("tracker's vote, 1 000 points", lambda t: t.count([frame], [-1]), walk_vote),
         ("cull, 40 key frames", lambda t: [(a, b) for a, b, _ in t.cull(cull_items)], walk_cull)]
for name, call, walk in cases:
    d, h, w = call(dev), call(twin), walk()
    equal = all(np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(a), np.asarray(c)) for a, b, c in zip(d, h, w))
    for _ in range(3):
        call(dev); call(twin)
    td, th, tw = [], [], []
    for r in range(reps):                                                # alternating, so that what else the machine does falls on all three
        a = time.perf_counter(); call(dev); b = time.perf_counter(); call(twin); c = time.perf_counter()
        td.append((b - a) * 1e3); th.append((c - b) * 1e3)
        if r < max(reps // 4, 3):                                        # the walk is slow: fewer repetitions
            walk(); tw.append((time.perf_counter() - c) * 1e3)
    pct = lambda t: [round(float(np.percentile(t, q)), 3) for q in (50, 10, 90)]
    print(name, json.dumps(dict(equal=bool(equal), device_ms_p50_p10_p90=pct(td), host_ms_p50_p10_p90=pct(th), dict_walk_ms_p50_p10_p90=pct(tw))), flush=True)
dev.close(); twin.close()
