"""GPU: the covisibility table on the device (csrc/covis_kernels.hip) equals the host twin, output for output and read-back for read-back, at the smallest shapes
that cross each seam: a partial last wave per row, more than one block of rows, the 64-bit seam of the query tags, item seams inside a wave, contended atomics.  The
twin itself is pinned to the literal loops in tests/test_covis_cpu.py, whose checks run here once more with the device."""
import ctypes as C

import numpy as np
import pytest

import covis_ref as R
import covis_scene as SC
import test_covis_cpu as T
from covis_scene import NLEVELS, SIND_E_CAPACITY

pytestmark = pytest.mark.gpu


def pair(cap_kf, cap_feat, cap_points, max_queries=64):
    return T.make(cap_kf, cap_feat, cap_points, True, max_queries), T.make(cap_kf, cap_feat, cap_points, False, max_queries)


def same_state(h, d):
    for k in range(h.cap_kf):
        assert all(np.array_equal(a, b) for a, b in zip(h.read_row(k), d.read_row(k))), k
    pts = np.arange(h.cap_points)
    assert all(np.array_equal(a, b) for a, b in zip(h.read_points(pts), d.read_points(pts)))


def same_counts(h, d, lists, self_kfs):
    a, b = h.count(lists, self_kfs), d.count(lists, self_kfs)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    return b


def same_culls(h, d, items):
    a, b = h.cull(items), d.cull(items)
    assert [(x[0], x[1], x[2].tolist()) for x in a] == [(x[0], x[1], x[2].tolist()) for x in b]
    return b


@pytest.mark.parametrize("shape", [(1, 1, 4, (1, 1, 1)), (3, 64, 50, (1, 64, 65, 40)), (70, 100, 300, (1, 64, 65, 3000))])
def test_table_shapes_and_op_counts(shape):
    """cap_feat 1, 64 and 100 (a partial last wave in each row); 1, 3 and 70 key frames (18 blocks of four rows); point ids 0 and cap_points - 1; batches of 1, 64 and 65 ops"""
    cap_kf, cap_feat, cap_points, batches = shape
    T.check_ops_against_the_model(False, *shape)
    h, d = pair(cap_kf, cap_feat, cap_points); rng = np.random.RandomState(cap_kf); model = R.Model(NLEVELS)
    first = [(cap_kf - 1, cap_feat - 1, cap_points - 1, NLEVELS - 1, 1)] + ([(0, 0, 0, 0, 0)] if cap_kf * cap_feat > 1 else [])
    fixed = {(f[0], f[1]) for f in first}                              # the two corner cells keep the lowest and the highest point id
    for n in (0,) + tuple(batches):
        ops = first if not n else [o for o in SC.random_ops(rng, model, cap_kf, cap_feat, cap_points, n, points=np.arange(1, cap_points - 1)) if (o[0], o[1]) not in fixed]
        SC.load(h, ops); SC.load(d, ops); model.apply(ops)
        same_state(h, d)
        pts = sorted({p for p, _, _ in model.cells.values()})
        lists = [np.array([cap_points - 1, 0, -1][:cap_feat]), rng.choice(pts, min(cap_feat, len(pts)), replace=False), rng.choice(pts, min(cap_feat, 7))]
        got = same_counts(h, d, lists, [-1, 0, cap_kf - 1])
        assert got[0][cap_kf - 1] == 1                                  # the point with the highest id in the last cell of the last row
        k = int(rng.randint(0, cap_kf)); row = model.row(k, cap_feat)
        same_culls(h, d, [(k, row[0], row[1], np.ones(cap_feat, np.uint8)), (cap_kf - 1, row[0][: cap_feat // 2], row[1][: cap_feat // 2], np.ones(cap_feat // 2, np.uint8))])
    h.close(); d.close()


def test_query_bits_across_the_64_bit_seam():
    """Q = 1, 64 and 65; 63 single-bit queries and then one of multiplicity 3, whose bits 63, 64, 65 straddle the seam; lists of 0 / 1 / 63 / 65 entries in one call"""
    ops, model = SC.random_table(3, 70, 100, 300); obs = model.observations(); rng = np.random.RandomState(4); pts = sorted(obs)
    h, d = pair(70, 100, 300, max_queries=128); SC.load(h, ops); SC.load(d, ops)
    lst = lambda n: rng.choice(pts, n, replace=False)
    for Q in (1, 64, 65):
        lists = [lst(int(rng.randint(1, 60))) for _ in range(Q)]; selfs = [int(rng.randint(-1, 70)) for _ in range(Q)]
        got = same_counts(h, d, lists, selfs)
        for l, s, g in zip(lists, selfs, got):
            assert np.array_equal(g, R.count_literal(l.tolist(), s, obs, 70))
    a, b = (int(x) for x in lst(2))
    lists = [lst(20) for _ in range(63)] + [np.array([a, b, a, a, b, -1] + lst(30).tolist())]
    got = same_counts(h, d, lists, [-1] * 64)
    assert np.array_equal(got[63], R.count_literal(lists[63].tolist(), -1, obs, 70)) and np.array_equal(got[0], R.count_literal(lists[0].tolist(), -1, obs, 70))
    lists = [lst(0), lst(1), lst(63), lst(65), np.full(9, -1)]
    got = same_counts(h, d, lists, [5, 5, -1, 0, 1])
    assert not got[0].any() and not got[4].any() and all(np.array_equal(g, R.count_literal(l.tolist(), s, obs, 70)) for l, s, g in zip(lists, [5, 5, -1, 0, 1], got))
    h.close(); d.close()


def test_count_repeated_and_after_interleaved_applies():
    ops, model = SC.random_table(5, 5, 100, 120); h, d = pair(6, 100, 130); SC.load(h, ops); SC.load(d, ops)
    rng = np.random.RandomState(6); lists = [rng.choice(120, 50, replace=False), np.array([3, 3, 3, 8, 8, 9])]
    first = same_counts(h, d, lists, [0, -1]); again = same_counts(h, d, lists, [0, -1])
    assert all(np.array_equal(a, b) for a, b in zip(first, again))      # the tags of the first call were cleared
    other = same_counts(h, d, [np.array([9, 8])], [-1])                  # and a different query sees none of them
    assert np.array_equal(other[0], R.count_literal([9, 8], -1, model.observations(), 6))
    cell = (5, 7)                                                        # a row nobody used yet: set, clear, set across calls
    for op, expect in (((5, 7, 125, 2, 1), 1), ((5, 7, -1, 0, 0), 0), ((5, 7, 125, 4, 0), 1), ((5, 7, 126, 1, 1), 0)):
        SC.load(h, [op]); SC.load(d, [op]); model.apply([op])
        got = same_counts(h, d, [np.array([125, 125])], [-1])[0]
        assert got[cell[0]] == 2 * expect and got.sum() == 2 * expect
        same_state(h, d)
    n_obs, hist = d.read_points([125, 126]); assert n_obs.tolist() == [0, 2] and not hist[0].any() and hist[1].tolist() == [0, 1] + [0] * 6
    h.close(); d.close()


def test_many_ops_on_one_point_in_one_call():
    """one point gets a cell in each of 70 key frames in ONE apply, and loses 69 of them and changes the last in another: its two aggregates take 70 atomics per call"""
    h, d = pair(70, 100, 10); rng = np.random.RandomState(8)
    ops = [(k, int(rng.randint(0, 100)), 7, int(rng.randint(0, NLEVELS)), k % 2) for k in range(70)]
    SC.load(h, ops); SC.load(d, ops); same_state(h, d)
    n_obs, hist = d.read_points([7]); assert n_obs[0] == 70 + 35 and hist.sum() == 70
    ops2 = [(k, i, -1, 0, 0) for k, i, _, _, _ in ops[:69]] + [(69, ops[69][1], 7, 5, 0)]
    SC.load(h, ops2); SC.load(d, ops2); same_state(h, d)
    n_obs, hist = d.read_points([7]); assert n_obs[0] == 1 and hist[0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    h.close(); d.close()


def test_cull_boundary_cases_on_the_device():
    T.check_cull_boundary_cases(False)


@pytest.mark.parametrize("shape", [(3, 1, 4, 1), (4, 64, 70, 5), (9, 100, 120, 5), (9, 100, 120, 1)])
def test_cull_batches_and_item_seams(shape):
    """B = 1 and 5 with n = cap_feat, 0, cap_feat / 2, 1, cap_feat: with cap_feat = 100 the items start at entries 0, 100, 100, 150 and 151, all inside a wave"""
    T.check_cull_against_the_literal_loop(False, 11 + shape[1], *shape)
    n_kf, cap_feat, n_points, B = shape
    ops, model = SC.random_table(40, n_kf, cap_feat, n_points, fill=0.8); h, d = pair(n_kf, cap_feat, n_points); SC.load(h, ops); SC.load(d, ops)
    rng = np.random.RandomState(41); items = []
    for b in range(B):
        k = int(rng.randint(0, n_kf)); n = [cap_feat, 0, cap_feat // 2, 1, cap_feat][b % 5]; row = model.row(k, cap_feat)
        items.append((k, np.where(rng.rand(n) < 0.1, -1, row[0][:n]), row[1][:n], (rng.rand(n) < 0.7).astype(np.uint8)))
    same_culls(h, d, items)
    h.close(); d.close()


def test_capacity_errors_leave_everything_untouched():
    from sindslam_amd.covisibility import _CullItem, _Query
    ops, model = SC.random_table(9, 3, 8, 20); t = T.make(3, 8, 20, False, max_queries=2); SC.load(t, ops)
    ptr = lambda x: C.c_void_p(x.ctypes.data)
    cnt = np.full(3, 77, np.int32); a = np.full(1, 77, np.int32); b = np.full(1, 77, np.int32); red = np.full(9, 77, np.uint8)

    def count(lists):
        arr = (_Query * len(lists))(); keep = [np.ascontiguousarray(l, np.int32) for l in lists]
        for q, l in zip(arr, keep):
            q.self_kf, q.n, q.points, q.count = -1, len(l), ptr(l), ptr(cnt)
        return t._fn("count")(t._h, arr, len(lists))

    def cull(ns):
        arr = (_CullItem * len(ns))(); pts = np.zeros(9, np.int32); o = np.zeros(9, np.uint8); c = np.ones(9, np.uint8)
        for it, n in zip(arr, ns):
            it.kf, it.n, it.points, it.octave, it.close, it.n_mps, it.n_redundant, it.redundant = 0, n, ptr(pts), ptr(o), ptr(c), ptr(a), ptr(b), ptr(red)
        return t._fn("cull")(t._h, arr, len(ns), 3)
    for name, call in (("Q > max_queries", lambda: count([[0]] * 3)), ("a list of more than cap_feat entries", lambda: count([np.arange(9)])),
                       ("B > max_queries", lambda: cull([1, 1, 1])),
                       ("an item of more than cap_feat entries", lambda: cull([9]))):
        assert call() == SIND_E_CAPACITY, name
        assert all((x == 77).all() for x in (cnt, a, b, red)), name
        SC.assert_state(t, model, range(3), range(20))
    t.close()
    t = T.make(2, 40, 5, False, max_queries=2); SC.load(t, [(0, 0, 1, 0, 0)])
    cnt = np.full(2, 77, np.int32)
    assert count([[1] * 40, [1] * 40]) == SIND_E_CAPACITY and (cnt == 77).all()      # 80 tag bits, 64 reserved
    assert count([[1] * 40, [1] * 24]) == 0 and cnt.tolist() == [24, 0]
    assert count([[1] * 3]) == 0 and cnt.tolist() == [3, 0]             # and the rejected call left no tag behind
    h = C.c_void_p()
    for args in ((1 << 15, 1 << 14, 20, 8, 4, 0), (3, 8, (1 << 24) + 1, 8, 4, 0), (3, 8, 20, 17, 4, 0), (3, 8, 20, 8, 4097, 0)):
        assert t._fn("create")(*args, C.byref(h)) == SIND_E_CAPACITY, args
    t.close()


def test_argument_errors_on_the_device():
    T.check_error_paths(False)
    from sindslam_amd._lib import lib
    assert len(lib().sind_last_error()) > 0


def test_python_layer_gives_the_dicts_of_the_cpu_run():
    dev, host = T.check_python_chain(False), T.check_python_chain(True)
    assert len(dev) == len(host) >= 8
    for a, b in zip(dev, host):
        SC.same_graph(a, b)
