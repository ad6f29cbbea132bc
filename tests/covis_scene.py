"""Scenes for the covisibility table (sindslam_amd.covisibility, include/sind_hip.h sind_covis_*): random op sequences and tables that keep the caller's contract (a
point has at most one cell per key frame), the hand-made boundary cases of the cull, lists for the count, and maps of plain dicts for the Python chain.  The checks
run the same scene on a table with host=True (the host twin) or host=False (the device)."""
import copy

import numpy as np

import covis_ref as R

SIND_E_ARG, SIND_E_CAPACITY = -1, -5
NLEVELS = 8


# ---- ops ----
def random_ops(rng, model, cap_kf, cap_feat, cap_points, n, p_clear=0.3, points=None):
    """n ops on distinct cells: clears (of occupied and of empty cells), sets of empty cells and replacements of occupied ones; a point never gets a second cell in
    a key frame.  The model is NOT changed.  -> list of (kf, idx, point, octave, stereo)"""
    cells = rng.choice(cap_kf * cap_feat, size=min(n, cap_kf * cap_feat), replace=False)
    in_row = {}
    for (k, idx), (p, _, _) in model.cells.items():
        in_row.setdefault(k, set()).add(p)
    ops = []
    for c in cells.tolist():
        k, idx = divmod(c, cap_feat)
        if rng.rand() < p_clear:
            ops.append((k, idx, -1, int(rng.randint(0, 99)), int(rng.randint(0, 2))))      # octave and stereo of a clear are not read
            continue
        row = in_row.setdefault(k, set())
        for _ in range(8):
            p = int(rng.choice(points)) if points is not None else int(rng.randint(0, cap_points))
            if p not in row:
                row.add(p); ops.append((k, idx, p, int(rng.randint(0, model.nlevels)), int(rng.randint(0, 2))))
                break
    return ops


def random_table(seed, n_kf, cap_feat, n_points, nlevels=NLEVELS, fill=0.6, dead=(), point_ids=None):
    """ops of a random map: every live key frame holds a random subset of the points at random indices -> (ops, model)"""
    rng = np.random.RandomState(seed); model = R.Model(nlevels); ops = []
    ids = np.arange(n_points) if point_ids is None else np.asarray(point_ids)
    for k in range(n_kf):
        if k in dead:
            continue
        n = min(int(round(fill * cap_feat)), len(ids))
        for idx, p in zip(rng.permutation(cap_feat)[:n].tolist(), rng.permutation(ids)[:n].tolist()):
            ops.append((k, idx, int(p), int(rng.randint(0, nlevels)), int(rng.randint(0, 2))))
    model.apply(ops)
    return ops, model


def load(table, ops, batch=None):
    """the ops through the raw apply, `batch` ops per call (None: all at once)"""
    from sindslam_amd.covisibility import _Op
    step = batch or max(len(ops), 1)
    for a in range(0, len(ops), step):
        part = ops[a:a + step]; arr = (_Op * len(part))(*part)
        assert table._fn("apply")(table._h, arr, len(part)) == 0


def assert_state(table, model, kfs, points):
    for k in kfs:
        got, ref = table.read_row(k), model.row(k, table.cap_feat)
        for g, r, name in zip(got, ref, ("point", "octave", "stereo")):
            assert np.array_equal(g, r), (k, name)
    n_obs, hist = table.read_points(points); rn, rh = model.points(list(points))
    assert np.array_equal(n_obs, rn) and np.array_equal(hist, rh)


# ---- count ----
def count_lists(rng, model, cap_points, self_kf):
    """the lists the issue names: plain, with -1 entries, one point named 1, 2 and 3 times, a point whose only cell is in self_kf, empty"""
    obs = model.observations(); pts = sorted(obs)
    only_self = [p for p in pts if list(obs[p]) == [self_kf]]
    a, b, c = (int(x) for x in rng.choice(pts, 3, replace=len(pts) < 3))
    return dict(plain=rng.choice(pts, min(40, len(pts)), replace=False), holes=np.where(rng.rand(min(40, len(pts))) < 0.4, -1, rng.choice(pts, min(40, len(pts)), replace=False)),
                multi=np.array([a, b, b, c, c, c, -1] + [int(x) for x in rng.choice(pts, 10)]), only_self=np.array(only_self[:1] + [a]), empty=np.zeros(0, np.int64),
                all_holes=np.full(5, -1), unknown=np.array([cap_points - 1, 0]))


# ---- cull: the boundary cases, worked out by hand ----
def cull_cases(nlevels=NLEVELS):
    """-> the ops of one table (6 key frames, 64 features, th_obs = 3) and {name: (kf, points, octave, close, expected (n_mps, n_redundant, redundant))}.  Key frame 0 is
    the one under test; every case has a point of its own, which is entry `i` of its list (the entries before it are -1), and its cells in the key frames 1 .. 4 sit at
    index 40 + its id."""
    ops, cases, top = [], {}, nlevels - 1

    def case(name, i, octave, own, others, expect, close=1):
        """own: None or (idx, octave, stereo) in key frame 0; others: (octave, stereo) per key frame 1 ..; expect: is the entry redundant"""
        p = len(cases)
        if own is not None:
            ops.append((0, own[0], p, own[1], own[2]))
        ops.extend((1 + k, 40 + p, p, o, s) for k, (o, s) in enumerate(others))
        cases[name] = (0, [-1] * i + [p], [0] * i + [octave], [1] * i + [close], (int(bool(close)), int(expect), [0] * i + [int(expect)]))
    case("exactly th_obs others is redundant", 0, 2, (0, 2, 0), [(2, 0)] * 3, True)
    case("th_obs - 1 others is not (n_obs 5)", 1, 2, (1, 2, 0), [(2, 1)] * 2, False)
    case("n_obs exactly 3 does not enter: a stereo and a mono cell", 2, 2, (2, 2, 1), [(2, 0)], False)
    case("two stereo cells, n_obs 4: enters, not redundant", 3, 2, (3, 2, 1), [(2, 1)], False)
    case("octave 0, the others at 1", 4, 0, (4, 0, 0), [(1, 0)] * 3, True)
    case("octave nlevels - 1: octave + 1 is clamped", 5, top, (5, top, 0), [(top, 0)] * 3, True)
    case("another key frame's cell at octave + 1 counts", 6, 3, (6, 3, 0), [(4, 0)] * 3, True)
    case("at octave + 2 it does not", 7, 3, (7, 3, 0), [(4, 0), (4, 0), (5, 0)], False)
    case("the own cell at another index of the row", 8, 2, (30, 2, 0), [(2, 0)] * 3, True)
    case("the own cell at another index, too coarse to be subtracted", 9, 2, (31, 7, 0), [(2, 0)] * 3, True)
    case("no own cell at all", 10, 2, None, [(2, 1)] * 3, True)
    case("no own cell, two others", 11, 2, None, [(2, 1)] * 2, False)
    case("the own cell does not count: two stereo others", 12, 2, (12, 2, 0), [(2, 1)] * 2, False)
    case("close = 0", 13, 2, (13, 2, 0), [(2, 0)] * 3, False, close=0)
    cases["n_mps = 0"] = (0, [-1, -1, 0], [0, 0, 2], [1, 0, 0], (0, 0, [0, 0, 0]))
    cases["an empty item"] = (0, [], [], [], (0, 0, []))
    return ops, cases


def cull_item(case):
    k, pts, octv, close, _ = case
    return k, np.array(pts, np.int32), np.array(octv, np.uint8), np.array(close, np.uint8)


# ---- maps of dicts for the Python chain ----
def toy_map(seed, n_kf=12, n_pts=400, cap_feat=100, nlevels=NLEVELS, reach=3.0):
    """n_kf key frames on a line; key frame k sees a point at position x with a probability that falls with |x - k| / reach; random indices and octaves, two thirds of
    the keypoints stereo with a depth of 0.5 .. 8, the others monocular (u_right = depth = -1).  Connections, parents and children as the reference builds them: every
    key frame runs UpdateConnections when it arrives, and takes its first parent then.  -> keyframes, mappoints"""
    from sindslam_amd import optimizer as O
    rng = np.random.RandomState(seed); x = rng.uniform(-1, n_kf, n_pts)
    mappoints = {m: dict(obs={}, bad=False) for m in range(n_pts)}; keyframes = {}
    for k in range(n_kf):
        see = np.nonzero(rng.rand(n_pts) < np.exp(-np.abs(x - k) / reach))[0]; see = rng.permutation(see)[:cap_feat]
        n = cap_feat; mp = np.full(n, -1, np.int64); idx = rng.permutation(n)[:len(see)]; mp[idx] = see
        stereo = rng.rand(n) < 0.67
        keyframes[k] = dict(mp=mp, octave=rng.randint(0, nlevels, n).astype(np.int32), u_right=np.where(stereo, rng.uniform(10, 600, n), -1).astype(np.float32),
                            depth=np.where(stereo, rng.uniform(0.5, 8, n), -1).astype(np.float32), bad=False, parent=None, children=set(), weights={}, covisible=[])
        for i, m in zip(idx.tolist(), see.tolist()):
            mappoints[m]["obs"][k] = i
    for k in range(n_kf):                                              # the map as it grows: observations of later key frames are not there yet
        part = {m: dict(p, obs={q: i for q, i in p["obs"].items() if q <= k}) for m, p in mappoints.items()}
        O.update_connections(k, keyframes, part)
        if k and keyframes[k]["covisible"]:
            keyframes[k]["parent"] = keyframes[k]["covisible"][0]; keyframes[keyframes[k]["parent"]]["children"].add(k)
    for m in list(mappoints)[::17]:
        mappoints[m]["bad"] = True
    for m, p in mappoints.items():
        p["ref_kf"] = min(p["obs"]) if p["obs"] else 0
    return keyframes, mappoints


def tracker_parent_break():
    """Key frames 0 .. 9; the frame's points vote for 3 and 4 alone.  Key frame 3: best neighbours [4, 2, 6] (4 is voted: 2 is taken), children {5} (taken), parent 1
    (taken: the break that ends the OUTER loop).  Key frame 4's neighbour 7, child 8 and parent 9 are therefore never taken.  -> keyframes, mappoints, frame_mp, expected"""
    keyframes = {k: dict(mp=np.full(4, -1, np.int64), octave=np.zeros(4, np.int32), u_right=np.full(4, -1, np.float32), depth=np.full(4, -1, np.float32), bad=False, parent=None,
                         children=set(), weights={}, covisible=[]) for k in range(10)}
    mappoints = {0: dict(obs={3: 0, 4: 0}, bad=False), 1: dict(obs={3: 1}, bad=False), 2: dict(obs={4: 1}, bad=False), 3: dict(obs={3: 2, 4: 2}, bad=True), 4: dict(obs={}, bad=False)}
    for m, p in mappoints.items():
        for k, i in p["obs"].items():
            keyframes[k]["mp"][i] = m
    keyframes[3].update(covisible=[4, 2, 6], children={5}, parent=1); keyframes[4].update(covisible=[3, 7], children={8}, parent=9)
    frame_mp = np.array([0, 1, -1, 1, 3, 4], np.int64)                 # point 1 twice (two votes for 3), a bad point, a point nobody observes
    return keyframes, mappoints, frame_mp, ([3, 4, 2, 5, 1], 3)


def tracker_more_than_80(voted):
    """`voted` key frames with one frame point each; key frame i has the unvoted neighbour 100 + i.  With 79 voted the loop takes 100 and 101 and stops at 81 > 80; with
    90 voted it takes nothing.  -> keyframes, mappoints, frame_mp"""
    keyframes = {k: dict(mp=np.full(1, -1, np.int64), octave=np.zeros(1, np.int32), u_right=np.full(1, -1, np.float32), depth=np.full(1, -1, np.float32), bad=False, parent=None,
                         children=set(), weights={}, covisible=[]) for k in range(100 + voted)}
    mappoints = {}
    for k in range(voted):
        mappoints[k] = dict(obs={k: 0}, bad=False); keyframes[k]["mp"][0] = k; keyframes[k]["covisible"] = [100 + k]
    frame_mp = np.array(list(range(voted)) + [7, 7], np.int64)        # key frame 7 gets three votes: the reference key frame
    return keyframes, mappoints, frame_mp


def culling_scene(nlevels=NLEVELS):
    """Key frames 0 .. 11 in a chain (parent k - 1), the current one 11.  Twenty points P are stereo cells at octave 2 in key frames 1, 2, 3, 4: each has exactly 3 cells in
    other key frames, so every one of the four is redundant AS THE MAP STANDS; once 1 is culled the others drop to 2 and 2, 3, 4 stay.  Twenty points R likewise in 6, 7,
    8, 10.  Point Z: a monocular cell in 1 and a stereo cell in 5 (nObs 3): culling 1 leaves nObs 2 and Z goes bad.  A few far and monocular keypoints are skipped by the
    depth test.  The literal loop culls 1 and 6; a single batch would cull all eight.  -> keyframes, mappoints, cur, th_depth"""
    from sindslam_amd import optimizer as O
    n = 40
    keyframes = {k: dict(mp=np.full(n, -1, np.int64), octave=np.full(n, 2, np.int32), u_right=np.full(n, 50.0, np.float32), depth=np.full(n, 2.0, np.float32), bad=False,
                         parent=(k - 1 if k else None), children=({k + 1} if k < 11 else set()), weights={}, covisible=[]) for k in range(12)}
    mappoints = {}

    def add(m, cells):
        mappoints[m] = dict(obs={}, bad=False)
        for k, i in cells:
            keyframes[k]["mp"][i] = m; mappoints[m]["obs"][k] = i
    for j in range(20):
        add(j, [(1, j), (2, j + 3), (3, j), (4, j + 5), (11, j)] if j < 16 else [(1, j), (2, j + 3), (3, j), (4, j + 5)])
        add(100 + j, [(6, j), (7, j + 1), (8, j), (10, j + 2), (11, 20 + j)] if j < 16 else [(6, j), (7, j + 1), (8, j), (10, j + 2)])
    for k in (1, 2, 3, 4, 6, 7, 8, 10):
        keyframes[k]["octave"][:] = 2
    add(200, [(1, 30), (5, 0)]); keyframes[1]["u_right"][30] = -1; keyframes[1]["depth"][30] = -1
    add(201, [(2, 35), (5, 1), (9, 0)]); keyframes[2]["depth"][35] = 100.0      # far: skipped
    add(202, [(5, 2), (9, 1), (11, 39)]); add(203, [(5, 3), (9, 2), (0, 0)])
    for k in sorted(keyframes):
        O.update_connections(k, keyframes, mappoints)
    # key frame 11 holds sixteen points of each group, so its covisible list names all eight (and 5 and 9 through 202)
    return keyframes, mappoints, 11, 40.0


def same_graph(a, b):
    """two maps (keyframes, mappoints) equal in everything the covisibility functions touch"""
    (ka, ma), (kb, mb) = a, b
    assert sorted(ka) == sorted(kb) and sorted(ma) == sorted(mb)
    for k in ka:
        assert np.array_equal(ka[k]["mp"], kb[k]["mp"]), k
        for key in ("bad", "parent", "children", "weights", "covisible", "to_be_erased", "track_ref_frame"):
            assert ka[k].get(key) == kb[k].get(key), (k, key, ka[k].get(key), kb[k].get(key))
    for m in ma:
        assert ma[m]["obs"] == mb[m]["obs"] and bool(ma[m].get("bad")) == bool(mb[m].get("bad")) and ma[m].get("ref_kf") == mb[m].get("ref_kf"), m


def table_of(keyframes, mappoints, host, cap_feat=None, max_queries=64):
    from sindslam_amd.covisibility import CovisibilityTable
    cap_feat = cap_feat or max(len(k["mp"]) for k in keyframes.values())
    return CovisibilityTable(max(keyframes) + 1, cap_feat, max(mappoints) + 1, NLEVELS, host=host, max_queries=max_queries).from_map(keyframes, mappoints)


def table_matches_map(table, keyframes, mappoints):
    """the table holds exactly the observations of the dicts"""
    model = R.Model(table.nlevels)
    model.apply([(k, i, m, int(keyframes[k]["octave"][i]), keyframes[k]["u_right"][i] >= 0) for m, p in mappoints.items() for k, i in p["obs"].items()])
    assert_state(table, model, sorted(keyframes), sorted(mappoints))


def clone(*maps):
    return tuple(copy.deepcopy(m) for m in maps)
