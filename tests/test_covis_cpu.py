"""CPU: the host twins sindh_covis_* (csrc/host/covis.hpp, the source the kernels of csrc/covis_kernels.hip compile too) against the literal loops of tests/covis_ref.py:
ops against a dict model, the count against the literal counter, the cull against the literal loop with its hand-made boundary cases; sindslam_amd.covisibility on toy
maps against the literal functions; the error paths; and a sanitizer build of the twin as a program of its own.  All of it is integer arithmetic: every comparison is
equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covis_ref as R
import covis_scene as SC
from covis_scene import NLEVELS, SIND_E_ARG

HOST = True                                                            # tests/test_covis_gpu.py runs the shared checks below with the device


def make(cap_kf, cap_feat, cap_points, host=HOST, max_queries=64, nlevels=NLEVELS):
    from sindslam_amd.covisibility import CovisibilityTable
    return CovisibilityTable(cap_kf, cap_feat, cap_points, nlevels, host=host, max_queries=max_queries)


# ---- checks shared with the GPU file: each takes host ----
def check_ops_against_the_model(host, cap_kf, cap_feat, cap_points, batches):
    rng = np.random.RandomState(cap_kf * 1000 + cap_feat); t = make(cap_kf, cap_feat, cap_points, host); model = R.Model(NLEVELS)
    from sindslam_amd.covisibility import _Op
    for n in batches:
        ops = SC.random_ops(rng, model, cap_kf, cap_feat, cap_points, n)
        SC.load(t, ops); model.apply(ops)
        SC.assert_state(t, model, range(cap_kf), sorted({0, cap_points - 1} | {p for p, _, _ in model.cells.values()}))
    if cap_feat > 1:
        before = [t.read_row(k) for k in range(cap_kf)]
        ops = [(0, 0, 0, 1, 0), (0, 1, 1, 1, 0), (0, 0, -1, 0, 0)]      # two ops on cell (0, 0)
        assert t._fn("apply")(t._h, (_Op * 3)(*ops), 3) == SIND_E_ARG
        for k in range(cap_kf):
            assert all(np.array_equal(a, b) for a, b in zip(before[k], t.read_row(k)))
        SC.assert_state(t, model, range(cap_kf), [0, cap_points - 1])
    t.clear(); SC.assert_state(t, R.Model(NLEVELS), range(cap_kf), [0, cap_points - 1])
    t.close()


def check_count_against_the_literal_counter(host, seed, n_kf, cap_feat, n_points, dead=()):
    cap_points = n_points + 3; lone = cap_points - 2
    ops, model = SC.random_table(seed, n_kf, cap_feat, n_points, dead=dead); self_kf = min(k for k in range(n_kf) if k not in dead)
    extra = [(max(k for k in range(n_kf) if k not in dead), 0, cap_points - 1, 0, 1)]      # the highest point id, replacing whatever the cell held
    if cap_feat > 1:
        extra.append((self_kf, int(np.nonzero(model.row(self_kf, cap_feat)[0][1:] < 0)[0][0]) + 1, lone, 1, 0))      # a point whose only cell is in self_kf
    model.apply(extra)
    t = make(n_kf + 2, cap_feat, cap_points, host); SC.load(t, ops); SC.load(t, extra)
    obs = model.observations(); rng = np.random.RandomState(seed + 1)
    lists = SC.count_lists(rng, model, cap_points, self_kf)
    lists = {k: np.asarray(v)[:cap_feat] for k, v in lists.items()}    # a list may hold cap_feat entries
    if cap_feat > 1:
        lists["lone"] = np.array([lone, int(lists["plain"][0])][:cap_feat])
    names = sorted(lists)
    for self_ in (self_kf, -1):
        got = t.count([lists[n] for n in names], [self_] * len(names))
        for n, g in zip(names, got):
            ref = R.count_literal(lists[n].tolist(), self_, obs, t.cap_kf)
            assert np.array_equal(g, ref), (n, self_, g, ref)
            if n in ("empty", "all_holes"):
                assert not g.any()
        one = t.count([lists["multi"]], [self_])[0]                    # and alone
        assert np.array_equal(one, got[names.index("multi")])
    if cap_feat > 1:
        assert t.count([lists["lone"]], [self_kf])[0].sum() == R.count_literal(lists["lone"].tolist(), self_kf, obs, t.cap_kf).sum()
        assert t.count([np.array([lone])], [self_kf])[0].sum() == 0 and t.count([np.array([lone])], [-1])[0][self_kf] == 1      # a point whose only cell is in self_kf
    for k in dead:
        assert all(g[k] == 0 for g in got)
    t.close()


def check_cull_boundary_cases(host):
    ops, cases = SC.cull_cases(); t = make(6, 64, 64, host); SC.load(t, ops)
    model = R.Model(NLEVELS); model.apply(ops)
    names = list(cases)
    for name in names:                                                 # one at a time: the expectation is the scene's, worked out by hand, and the literal loop agrees
        k, pts, octv, close, (n_mps, n_red, flags) = cases[name]
        got = t.cull([SC.cull_item(cases[name])])[0]
        assert (got[0], got[1], got[2].tolist()) == (n_mps, n_red, flags), (name, got)
        lit = R.cull_literal(k, pts, octv, close, model)
        assert (lit[0], lit[1], lit[2].tolist()) == (n_mps, n_red, flags), (name, lit)
    got = t.cull([SC.cull_item(cases[n]) for n in names])             # all of them as one batch: unequal n, 0 included
    assert [(g[0], g[1], g[2].tolist()) for g in got] == [cases[n][4] for n in names]
    merged = np.full(16, -1, np.int32); octv = np.zeros(16, np.uint8); close = np.ones(16, np.uint8)      # and as ONE item: every case's entry at its own index
    for n in names[:14]:
        _, p, o, c, _ = cases[n]; i = len(p) - 1; merged[i], octv[i], close[i] = p[i], o[i], c[i]
    g = t.cull([(0, merged, octv, close)])[0]
    assert g[0] == sum(cases[n][4][0] for n in names[:14]) and g[1] == sum(cases[n][4][1] for n in names[:14]) and g[2].sum() == g[1]
    t.close()


def check_cull_against_the_literal_loop(host, seed, n_kf, cap_feat, n_points, B):
    ops, model = SC.random_table(seed, n_kf, cap_feat, n_points, fill=0.8); t = make(n_kf, cap_feat, n_points, host); SC.load(t, ops)
    rng = np.random.RandomState(seed + 7); items = []
    for b in range(B):
        k = int(rng.randint(0, n_kf)); n = [cap_feat, 0, cap_feat // 2, 1, cap_feat][b % 5]
        pts = model.row(k, cap_feat)[0][:n].copy(); octv = model.row(k, cap_feat)[1][:n].copy()
        swap = rng.rand(n) < 0.15; pts[swap] = rng.randint(0, n_points, int(swap.sum())); octv[swap] = rng.randint(0, NLEVELS, int(swap.sum()))      # an inconsistent map: points of other rows
        items.append((k, pts, octv, (rng.rand(n) < 0.8).astype(np.uint8)))
    got = t.cull(items)
    for it, g in zip(items, got):
        lit = R.cull_literal(it[0], it[1].tolist(), it[2].tolist(), it[3].tolist(), model)
        assert (g[0], g[1]) == (lit[0], lit[1]) and np.array_equal(g[2], lit[2]), (it[0], g, lit)
    assert sum(g[1] for g in got) > 0 or cap_feat < 8
    t.close()


def check_python_chain(host):
    """-> the dicts after the three functions, for the GPU file to compare with the CPU run"""
    from sindslam_amd import covisibility as CV
    from sindslam_amd import optimizer as O
    out = []
    # update_connections_many = the sequence of optimizer.update_connections
    kfs, mps = SC.toy_map(3)
    for k in kfs:                                                      # the map moved on since the connections were made: points went bad, and a fusion replaced some
        kfs[k]["weights"] = dict(list(kfs[k]["weights"].items())[:2]); kfs[k]["covisible"] = kfs[k]["covisible"][:1]
    (ka, ma), (kb, mb) = SC.clone(kfs, mps), SC.clone(kfs, mps)
    t = SC.table_of(ka, ma, host, max_queries=5)                       # 12 key frames in batches of 5
    CV.update_connections_many(t, sorted(ka), ka, ma)
    for k in sorted(kb):
        O.update_connections(k, kb, mb)
    SC.same_graph((ka, ma), (kb, mb)); assert any(len(k["covisible"]) > 1 for k in ka.values()) and any(min(k["weights"].values(), default=99) < 15 for k in ka.values())
    out.append((ka, ma)); t.close()
    # update_local_keyframes: the parent break, and the stop at more than 80
    kfs, mps, frame_mp, expected = SC.tracker_parent_break()
    (ka, ma), (kb, mb) = SC.clone(kfs, mps), SC.clone(kfs, mps); fa, fb = frame_mp.copy(), frame_mp.copy()
    t = SC.table_of(ka, ma, host, cap_feat=len(frame_mp))             # the frame's list may hold cap_feat entries
    got = CV.update_local_keyframes(t, fa, ka, ma, 77); lit = R.update_local_keyframes(fb, kb, mb, 77)
    assert got == lit == expected and np.array_equal(fa, fb) and fa[4] == -1
    assert 7 not in got[0] and 8 not in got[0] and 9 not in got[0]     # the break after the parent left the outer loop: key frame 4 was never expanded
    SC.same_graph((ka, ma), (kb, mb)); out.append((ka, ma))
    assert CV.update_local_keyframes(t, np.array([-1, 4]), ka, ma, 78) == (None, None) == R.update_local_keyframes(np.array([-1, 4]), kb, mb, 78)
    t.close()
    for voted, n_local in ((79, 81), (90, 90)):
        kfs, mps, frame_mp = SC.tracker_more_than_80(voted)
        (ka, ma), (kb, mb) = SC.clone(kfs, mps), SC.clone(kfs, mps)
        t = SC.table_of(ka, ma, host, cap_feat=max(len(frame_mp), 1))
        got = CV.update_local_keyframes(t, frame_mp.copy(), ka, ma, 5); lit = R.update_local_keyframes(frame_mp.copy(), kb, mb, 5)
        assert got == lit and len(got[0]) == n_local and got[1] == 7 and got[0][:voted] == list(range(voted)) and got[0][voted:] == [100, 101][:n_local - voted]
        out.append((ka, ma)); t.close()
    kfs, mps = SC.toy_map(4)
    (ka, ma), (kb, mb) = SC.clone(kfs, mps), SC.clone(kfs, mps); rng = np.random.RandomState(9)
    frame_mp = np.concatenate([kfs[5]["mp"][:60], rng.randint(0, len(mps), 40)])      # what the frame tracked of key frame 5, and some more: duplicates happen
    t = SC.table_of(ka, ma, host)
    got = CV.update_local_keyframes(t, frame_mp.copy(), ka, ma, 9); lit = R.update_local_keyframes(frame_mp.copy(), kb, mb, 9)
    assert got == lit and got[1] == 5 and len(got[0]) >= 5
    t.close()
    # keyframe_culling: a cull that flips the verdict of a later key frame, and one that makes a point bad
    kfs, mps, cur, th = SC.culling_scene()
    (ka, ma), (kb, mb), (kc, mc) = SC.clone(kfs, mps), SC.clone(kfs, mps), SC.clone(kfs, mps)
    t = SC.table_of(ka, ma, host)
    got = CV.keyframe_culling(t, cur, ka, ma, th); lit = R.keyframe_culling(cur, kb, mb, th)
    assert got == lit == [1, 6]
    SC.same_graph((ka, ma), (kb, mb)); SC.table_matches_map(t, ka, ma)
    assert ma[200]["bad"] and not ma[200]["obs"] and ka[5]["mp"][0] == -1 and not mps[200]["bad"]      # the cull of key frame 1 took point 200 to nObs 2
    assert ka[2]["parent"] == 0 and 2 in ka[0]["children"] and 1 not in ka[0]["children"]      # the child of the culled key frame went to its parent
    t2 = SC.table_of(kc, mc, host)
    alone = CV.keyframe_culling(t2, cur, kc, mc, th, replay=False)
    assert alone != lit and set(alone) > set(lit)                      # the scene's property: one batch without replay culls key frames the literal loop keeps
    out.append((ka, ma)); t.close(); t2.close()
    for th_depth in (None, 4.0):                                       # and a map where little or nothing is culled, monocular and RGB-D
        kfs, mps = SC.toy_map(6, n_kf=8, n_pts=150, reach=6.0)
        (ka, ma), (kb, mb) = SC.clone(kfs, mps), SC.clone(kfs, mps)
        kb[3]["not_erase"] = ka[3]["not_erase"] = True
        t = SC.table_of(ka, ma, host)
        assert CV.keyframe_culling(t, 7, ka, ma, th_depth) == R.keyframe_culling(7, kb, mb, th_depth)
        SC.same_graph((ka, ma), (kb, mb)); SC.table_matches_map(t, ka, ma); out.append((ka, ma)); t.close()
    # set_bad_flag alone, and the table's own map operations
    kfs, mps = SC.toy_map(8)
    (ka, ma), (kb, mb) = SC.clone(kfs, mps), SC.clone(kfs, mps)
    t = SC.table_of(ka, ma, host)
    for k in (0, 4, 6):
        assert CV.set_bad_flag(t, k, ka, ma) == (k != 0); R.set_bad_flag(k, kb, mb)
    SC.same_graph((ka, ma), (kb, mb)); SC.table_matches_map(t, ka, ma)
    assert not ka[0]["bad"] and ka[4]["bad"] and any(ma[m]["bad"] and not mps[m]["bad"] for m in ma)
    old, new = next((a, b) for a in ma for b in ma if a != b and ma[a]["obs"] and ma[b]["obs"] and set(ma[a]["obs"]) & set(ma[b]["obs"]) and set(ma[a]["obs"]) - set(ma[b]["obs"]))
    t.replace(ma[old]["obs"], new, ma[new]["obs"], ka); O._replace(ka, ma, old, new); SC.table_matches_map(t, ka, ma)
    t.erase_keyframe(2)
    for m in ma.values():
        m["obs"].pop(2, None)
    SC.table_matches_map(t, ka, ma); out.append((ka, ma)); t.close()
    return out


# ---- the CPU tests ----
@pytest.mark.parametrize("shape", [(1, 1, 4, (1, 1, 1)), (3, 64, 50, (1, 64, 65, 40)), (7, 100, 300, (200, 300, 65, 700))])
def test_ops_equal_the_dict_model(shape):
    check_ops_against_the_model(HOST, *shape)


@pytest.mark.parametrize("shape", [(1, 1, 6, ()), (3, 64, 90, ()), (9, 100, 260, (0, 4, 8))])
def test_count_equals_the_literal_counter(shape):
    seed = shape[1]
    check_count_against_the_literal_counter(HOST, seed, *shape[:3], dead=shape[3])


def test_cull_boundary_cases():
    check_cull_boundary_cases(HOST)


@pytest.mark.parametrize("shape", [(3, 1, 4, 1), (4, 64, 70, 5), (9, 100, 120, 5)])
def test_cull_equals_the_literal_loop(shape):
    check_cull_against_the_literal_loop(HOST, 11 + shape[1], *shape)


def test_python_chain_equals_the_literal_functions():
    check_python_chain(HOST)


def error_calls(t):
    """every entry point with a bad argument -> (name, call, expected code, the arrays that must stay untouched)"""
    from sindslam_amd.covisibility import _CullItem, _Op, _Query
    F, P, K = t.cap_feat, t.cap_points, t.cap_kf
    pts = np.array([0, 1], np.int32); cnt = np.full(K, 77, np.int32); octv = np.zeros(2, np.uint8); close = np.ones(2, np.uint8)
    a = np.full(1, 77, np.int32); b = np.full(1, 77, np.int32); red = np.full(2, 77, np.uint8)
    ptr = lambda x: C.c_void_p(x.ctypes.data)
    out = []
    for name, op in (("kf", (K, 0, 0, 0, 0)), ("kf negative", (-1, 0, 0, 0, 0)), ("idx", (0, F, 0, 0, 0)), ("point", (0, 0, P, 0, 0)), ("point below -1", (0, 0, -2, 0, 0)),
                     ("octave", (0, 0, 0, NLEVELS, 0)), ("octave negative", (0, 0, 0, -1, 0))):
        out.append(("apply: " + name, lambda op=op: t._fn("apply")(t._h, (_Op * 2)((1, 0, 1, 0, 0), op), 2), SIND_E_ARG))
    out.append(("apply: null", lambda: t._fn("apply")(t._h, None, 2), SIND_E_ARG)); out.append(("apply: negative n", lambda: t._fn("apply")(t._h, (_Op * 1)(), -1), SIND_E_ARG))
    out.append(("apply: null handle", lambda: t._fn("apply")(None, (_Op * 1)(), 1), SIND_E_ARG))

    def count(self_kf=0, n=2, points=pts, out_=cnt, Q=2, null=False):
        arr = (_Query * 2)(); arr[0].self_kf, arr[0].n, arr[0].points, arr[0].count = 0, 2, ptr(pts), ptr(cnt)
        arr[1].self_kf, arr[1].n, arr[1].points, arr[1].count = self_kf, n, (ptr(points) if points is not None else None), (ptr(out_) if out_ is not None else None)
        return t._fn("count")(t._h, None if null else arr, Q)
    for name, kw in (("self_kf", dict(self_kf=K)), ("self_kf below -1", dict(self_kf=-2)), ("negative n", dict(n=-1)), ("null points", dict(points=None)), ("null count", dict(out_=None)),
                     ("point", dict(points=np.array([0, P], np.int32))), ("point below -1", dict(points=np.array([-2, 0], np.int32))), ("negative Q", dict(Q=-1)), ("null queries", dict(null=True))):
        out.append(("count: " + name, lambda kw=kw: count(**kw), SIND_E_ARG))

    def cull(kf=0, n=2, points=pts, octave=octv, close_=close, n_mps=a, B=2, null=False):
        arr = (_CullItem * 2)()
        for it in arr:
            it.kf, it.n, it.points, it.octave, it.close, it.n_mps, it.n_redundant, it.redundant = 0, 2, ptr(pts), ptr(octv), ptr(close), ptr(a), ptr(b), ptr(red)
        it = arr[1]; it.kf, it.n = kf, n
        it.points = ptr(points) if points is not None else None; it.octave = ptr(octave) if octave is not None else None; it.close = ptr(close_) if close_ is not None else None
        it.n_mps = ptr(n_mps) if n_mps is not None else None
        return t._fn("cull")(t._h, None if null else arr, B, 3)
    for name, kw in (("kf", dict(kf=K)), ("kf negative", dict(kf=-1)), ("negative n", dict(n=-1)), ("null points", dict(points=None)), ("null octave", dict(octave=None)), ("null close", dict(close_=None)),
                     ("null n_mps", dict(n_mps=None)), ("point", dict(points=np.array([P, 0], np.int32))), ("octave", dict(octave=np.array([0, NLEVELS], np.uint8))), ("negative B", dict(B=-1)),
                     ("null items", dict(null=True))):
        out.append(("cull: " + name, lambda kw=kw: cull(**kw), SIND_E_ARG))
    row = (np.full(F, 77, np.int32), np.full(F, 77, np.uint8), np.full(F, 77, np.uint8)); no = np.full(2, 77, np.int32); hist = np.full((2, NLEVELS), 77, np.int32)
    out.append(("read_row: kf", lambda: t._fn("read_row")(t._h, K, ptr(row[0]), ptr(row[1]), ptr(row[2])), SIND_E_ARG))
    out.append(("read_row: null", lambda: t._fn("read_row")(t._h, 0, None, ptr(row[1]), ptr(row[2])), SIND_E_ARG))
    out.append(("read_points: point", lambda: t._fn("read_points")(t._h, ptr(np.array([0, P], np.int32)), 2, ptr(no), ptr(hist)), SIND_E_ARG))
    out.append(("read_points: null", lambda: t._fn("read_points")(t._h, ptr(pts), 2, None, ptr(hist)), SIND_E_ARG))
    out.append(("clear: null handle", lambda: t._fn("clear")(None), SIND_E_ARG))
    return out, (cnt, a, b, red, row[0], row[1], row[2], no, hist)


def check_error_paths(host):
    ops, model = SC.random_table(5, 3, 8, 20); t = make(3, 8, 20, host); SC.load(t, ops)
    calls, untouched = error_calls(t)
    for name, call, code in calls:
        assert call() == code, name
        assert all((x == 77).all() for x in untouched), name
        SC.assert_state(t, model, range(3), range(20))
    h = C.c_void_p()
    for args, code in (((0, 8, 20, 8, 4, 0), SIND_E_ARG), ((3, 0, 20, 8, 4, 0), SIND_E_ARG), ((3, 8, 0, 8, 4, 0), SIND_E_ARG), ((3, 8, 20, 0, 4, 0), SIND_E_ARG), ((3, 8, 20, 17, 4, 0), SC.SIND_E_CAPACITY)):
        assert t._fn("create")(*args, C.byref(h)) == code, args
    assert t._fn("create")(3, 8, 20, 8, 4, 0, None) == SIND_E_ARG
    assert t._fn("apply")(t._h, None, 0) == 0 and t._fn("count")(t._h, None, 0) == 0 and t._fn("cull")(t._h, None, 0, 3) == 0      # n = 0, Q = 0 and B = 0 are valid
    t.close()


def test_argument_errors_leave_everything_untouched():
    check_error_paths(HOST)


def test_the_queue_flushes_when_a_cell_is_met_twice():
    t = make(2, 4, 8)
    t.add_observation(0, 1, 3, 2, True); t.add_observation(1, 1, 3, 0, False); assert len(t._ops) == 2
    t.erase_observation(0, 1); assert len(t._ops) == 1                   # the second op on cell (0, 1) sent the first two off
    t.add_observation(0, 1, 5, 1, False); assert len(t._ops) == 1
    n_obs, hist = t.read_points([3, 5]); assert not t._ops
    assert n_obs.tolist() == [1, 1] and hist[0].tolist() == [1] + [0] * 7 and t.read_row(0)[0].tolist() == [-1, 5, -1, -1]
    t.close()


def test_a_sanitizer_build_of_the_host_twin_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_covis_* and csrc/host/covis.cpp with -fsanitize=address,undefined, run as a program of its own on the scenes of this file: random ops with a
    rejected call, the count lists, the cull boundary cases and a random cull"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "covis_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "sindslam_amd", "csrc"), "sanitize-covis", "OUT=" + exe], check=True, capture_output=True, text=True)
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    rec, expect = [], []
    cap_kf, cap_feat, cap_points = 5, 100, 130
    ops, model = SC.random_table(21, 4, cap_feat, 120); rng = np.random.RandomState(22)
    t = make(cap_kf, cap_feat, cap_points)
    more = SC.random_ops(rng, model, cap_kf, cap_feat, cap_points, 90)
    for part, rc in ((ops, 0), (more, 0), ([(0, 0, 1, 0, 0), (0, 0, 2, 0, 0)], SIND_E_ARG), ([], 0)):
        rec.append(i32(0, rc, len(part)) + np.array(part, np.int32).reshape(-1, 5).tobytes())
        if rc == 0:
            SC.load(t, part); model.apply(part)
        n_obs, hist = t.read_points(np.arange(cap_points))
        expect.append([rc, int(n_obs.sum()), int((hist * np.arange(1, NLEVELS + 1)).sum()), int(sum(int(t.read_row(k)[0].astype(np.int64).sum()) for k in range(cap_kf)))])
    lists = SC.count_lists(rng, model, cap_points, 1)
    for name in sorted(lists):
        pts = np.asarray(lists[name], np.int32)
        for self_kf in (1, -1):
            rec.append(i32(1, 0, self_kf, len(pts)) + pts.tobytes()); g = t.count([pts], [self_kf])[0]
            expect.append([0, int(g.sum()), int((g * np.arange(1, cap_kf + 1)).sum())])
    rec.append(i32(1, SIND_E_ARG, 0, 1) + i32(cap_points)); expect.append([SIND_E_ARG])
    items = []
    for b in range(3):
        k = b; n = (cap_feat, 0, 37)[b]; pts = model.row(k, cap_feat)[0][:n].copy(); pts[::5] = rng.randint(0, 120, len(pts[::5]))
        items.append((k, pts, rng.randint(0, NLEVELS, n).astype(np.uint8), (rng.rand(n) < 0.8).astype(np.uint8)))
    for (k, pts, octv, close), g in zip(items, t.cull(items)):
        rec.append(i32(2, 0, k, len(pts)) + pts.tobytes() + octv.tobytes() + close.tobytes()); expect.append([0, g[0], g[1], int(g[2].sum())])
    rec.append(i32(2, SIND_E_ARG, cap_kf, 0)); expect.append([SIND_E_ARG])
    t.close()
    ops2, cases = SC.cull_cases(); t = make(6, 64, 64); SC.load(t, ops2)      # and the boundary cases of the cull, on their own table
    n_obs, hist = t.read_points(np.arange(64))
    rec2 = [i32(0, 0, len(ops2)) + np.array(ops2, np.int32).tobytes()]
    expect2 = [[0, int(n_obs.sum()), int((hist * np.arange(1, NLEVELS + 1)).sum()), int(sum(int(t.read_row(k)[0].astype(np.int64).sum()) for k in range(6)))]]
    for name, case in cases.items():
        k, pts, octv, close = SC.cull_item(case)
        rec2.append(i32(2, 0, k, len(pts)) + pts.tobytes() + octv.tobytes() + close.tobytes()); expect2.append([0, case[4][0], case[4][1], sum(case[4][2])])
    t.close()
    for tag, dims, records, expected in (("a", (cap_kf, cap_feat, cap_points), rec, expect), ("b", (6, 64, 64), rec2, expect2)):
        path = tmp_path / f"records_{tag}.bin"
        with open(path, "wb") as f:
            f.write(i32(*dims, NLEVELS, len(records))); f.write(b"".join(records))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (tag, r.returncode, r.stderr[-2000:])
        lines = [[int(v) for v in line.split()] for line in r.stdout.split("\n")[:-1]]
        assert lines == expected, tag
