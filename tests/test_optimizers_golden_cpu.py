"""CPU: every output of the host twins of the three optimizers (sindh_pose_optimize, sindh_sim3_optimize, sindh_local_ba; csrc/host/pose_opt.hpp, sim3_opt.hpp,
local_ba.hpp over g2o_lm.hpp), diagnostics included, against tests/golden/optimizers_host.npz as bit patterns.  The fixture was recorded from the host library as it
was before the three optimizers were put on one Levenberg-Marquardt driver and one LDLT, over the sizes at which the shared code takes another path (the 64- and
128-edge chunks of the device twins, the n < 3 / n < 10 early returns, the empty graph) and the degenerate scenes of the three test_*_cpu.py files.  The Python
restatements stay the independent pin of WHAT is computed; this pins THAT it did not move, on many more sizes than they can cover in the time a test has."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizers_host.npz")


def pose_cases():
    import poseopt_scene as P
    for n in (2, 3, 9, 10, 63, 64, 65, 127, 128, 129):
        for kind in ("mono", "stereo", "mixed"):
            yield f"pose/{n}/{kind}", P.scene(n + {"mixed": 0, "mono": 100, "stereo": 200}[kind], n, kind)
    yield "pose/depth_zero", P.behind_camera()
    yield "pose/identical_mono", P.identical_points()
    yield "pose/identical_stereo", P.identical_points(stereo=True)


def sim3_cases():
    """-> name, scene, fix_scale"""
    import sim3opt_scene as SC
    for n in (0, 9, 10, 31, 32, 33, 64, 65, 129):
        for fix in (True, False):
            for outliers in (0.0, 0.3):
                yield f"sim3/{n}/{int(fix)}/{outliers}", SC.scene(n + (50 if fix else 0), n, outliers=outliers, scale=1.0 if fix else 0.93, start=(0.03, 0.03, 0.0 if fix else -0.04)), fix
    for name, s in SC.degenerates().items():
        for fix in (True, False):
            yield f"sim3/{name}/{int(fix)}", s, fix


def localba_cases():
    """the scenes of test_localba_cpu.py; its literal cases hold the degenerate ones: a depth of zero, no observation (no active vertex), no point (an empty graph)"""
    import localba_scene as SC
    for kind in ("mono", "stereo", "mixed"):
        for seed in (2, 21):
            yield f"lba/{seed}/{kind}", SC.scene(seed, 3, 1, 30, kind=kind, outliers=4, obs_per_point=3 if seed == 21 else None, id0=seed == 21)
        yield f"lba/planted/{kind}", SC.scene(7, 6, 2, 30, kind=kind, outliers=5)
    for seed, kind in ((31, "mono"), (32, "stereo"), (33, "mixed"), (34, "mixed")):
        yield f"lba/{seed}/{kind}", SC.scene(seed, 4, 1, 30, kind=kind, outliers=3, obs_per_point=None if seed < 34 else 3)
    for seed, kind in ((51, "mono"), (52, "stereo"), (53, "mixed")):
        yield f"lba/{seed}/{kind}", SC.scene(seed, 3, 1, 14, kind=kind, outliers=2)
    for name, s in SC.literal_cases().items():
        yield f"lba/{name}", s


def outputs():
    """every output array of every case from the built host library -> {"case/output": array}"""
    import localba_scene as LS
    import poseopt_scene as PS
    import sim3opt_scene as SS
    out = {}
    for name, s in pose_cases():
        r = PS.HostOptimizer().PoseOptimization([s])[0]
        out.update({f"{name}/{k}": np.asarray(r[k]) for k in PS.OUTPUTS})
    for name, s, fix in sim3_cases():
        r = SS.HostOptimizer().OptimizeSim3([s], 10, fix)[0]
        out.update({f"{name}/{k}": np.asarray(r[k]) for k in SS.OUTPUTS})
    for name, s in localba_cases():
        r = LS.HostBA().LocalBundleAdjustment([s])[0]
        out.update({f"{name}/{k}": np.asarray(r[k]) for k in LS.OUTPUTS})
    return out


def raw(a):
    """the bit patterns of an array: floats as unsigned integers of their width, so that a NaN equals only the same NaN and -0.0 differs from 0.0"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def pack(arrays):
    """{name: array} as the fixture holds it: the names, each array's dtype and shape, and per dtype one vector of all its arrays' bit patterns in the order of the names"""
    names = sorted(arrays)
    out = dict(names=np.array(names), dtypes=np.array([arrays[k].dtype.str for k in names]), shapes=np.array(["x".join(map(str, arrays[k].shape)) for k in names]))
    for d in sorted(set(out["dtypes"])):
        out["bits" + d] = np.concatenate([raw(arrays[k]).reshape(-1) for k in names if arrays[k].dtype.str == d])
    return out


def test_host_optimizers_reproduce_the_recorded_outputs_bit_for_bit():
    got = outputs()
    with np.load(GOLDEN) as f:
        gold = {k: f[k] for k in f.files}
    assert list(gold["names"]) == sorted(got)
    assert sum(int(np.isnan(gold[k].view(np.float64)).sum()) for k in gold if k.startswith("bits") and k.endswith("f8")) >= 6      # the NaN systems are among the recorded
    mine = pack(got)
    assert sorted(mine) == sorted(gold)
    for k in ("dtypes", "shapes"):
        assert np.array_equal(mine[k], gold[k]), [(n, a, b) for n, a, b in zip(gold["names"], gold[k], mine[k]) if a != b][:8]
    at = {}
    for name, d, shape in zip(gold["names"], gold["dtypes"], gold["shapes"]):      # per array, so that a failure names the case and the output
        n = int(np.prod([int(v) for v in shape.split("x")])) if shape else 1
        lo = at.get(d, 0); at[d] = lo + n
        assert np.array_equal(gold["bits" + d][lo:lo + n], mine["bits" + d][lo:lo + n]), (name, got[name])
