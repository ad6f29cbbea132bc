"""Timing of sind_match_pnp_ransac, the recipe of profiles/match_pnp_ransac.txt (argument `device`: the device call alone, fewer repetitions, for a kernel trace): 20 candidates of n about 100, 30 % outliers, Relocalisation's parameters (35 iterations at most),
and the same candidates with 300 iterations; the device call against the same schedule through the host entry points.  200 timed repetitions after 10."""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_cases as H, pnp_scene as S, sim3_scene as S3
from sindslam_amd import pnp
from sindslam_amd.matcher import ORBmatcher

only_device = len(sys.argv) > 1 and sys.argv[1] == "device"
reps = 30 if only_device else 200
mt = ORBmatcher(*[float(k) for k in S.K], 40.0, (0, 640, 0, 480), S3.scale_factors(), cap=256, max_batch=20)
rng = np.random.default_rng(0)
inps = [S.candidate(500 + b, 90 + b, outliers=0.3, noise=0.5) for b in range(20)]
out = {}
for its in (35, 300):
    req = []
    for inp in inps:
        n = len(inp["sigma2"]); mi, mx = pnp.ransac_params(n, 0.99, 10, 300, 4, 0.5)
        k = min(its, mx) if its == 35 else its
        req.append((inp, np.stack([rng.choice(n, 4, replace=False) for _ in range(k)]).astype(np.int32), mi, 0, None))
    def timed(f, r):
        for _ in range(10 if r > 20 else 2): f()
        t = []
        for _ in range(r):
            a = time.perf_counter(); f(); t.append((time.perf_counter() - a) * 1e3)
        return [float(np.percentile(t, q)) for q in (50, 10, 90)]
    got = mt.PnPRansac(req)
    res = dict(iterations=[len(r[1]) for r in req][:3], refines=int(sum(len(g["refine_hyp"]) for g in got)), device_ms_p50_p10_p90=timed(lambda: mt.PnPRansac(req), reps))
    if not only_device:
        host = H.host_evaluate(S.K)
        res["host_ms_p50_p10_p90"] = timed(lambda: host(req), 200 if its == 35 else 20)
        ref = host(req)
        res["equal"] = all(np.array_equal(H.bits64(g["R"]), H.bits64(r["R"])) and np.array_equal(g["count"], r["count"]) and np.array_equal(H.bits64(g["refine_t"]), H.bits64(r["refine_t"])) for g, r in zip(got, ref))
    out[its] = res
    print(its, json.dumps(res), flush=True)
mt.close()
