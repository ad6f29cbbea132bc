"""GPU: sind_match_essential_graph (csrc/match_essgraph.hip: k_ess_graph, k_ess_points) against its host twin sindh_essential_graph, which compiles the same
csrc/host/essential_graph.hpp: every output and diagnostic as bit patterns.  The host twin itself is pinned by tests/test_essgraph_cpu.py.  T below is ESS_THREADS,
the workgroup size of k_ess_graph; a full grid of k_ess_points is ESS_PT_BLOCKS x ESS_PT_THREADS = 16384 points per item."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 512
PT = 256                                                                     # ESS_PT_THREADS, the workgroup size of k_ess_points
FULL_GRID = 64 * 256                                                         # ESS_PT_BLOCKS x ESS_PT_THREADS
SIND_E_ARG, SIND_E_CAPACITY = -1, -5
_cache = {}


def _matcher(max_batch=4):
    from sindslam_amd.matcher import ORBmatcher
    return ORBmatcher(520.0, 516.0, 320.0, 240.0, 40.0, (0.0, 640.0, 0.0, 480.0), [1.2 ** k for k in range(8)], cap=512, max_batch=max_batch)


def _scenes():
    """the parity scenes, built once: name -> item.  7 K' is the size of the system, K' the free key frames with an edge (all but the fixed one)."""
    if "scenes" not in _cache:
        import essgraph_scene as S
        sc = {}
        sc["kf2"] = S.scene(31, 2, window=1, loop=1, n_mp=1)                    # one free vertex: 7 unknowns, three edges to the fixed one
        sc["kf3"] = S.scene(32, 3, window=2, loop=1, n_mp=0)
        sc["kf10"] = S.scene(33, 10, window=3, loop=2, n_mp=T - 1)              # 7 K' = 63
        sc["kf11"] = S.scene(34, 11, window=3, loop=2, n_mp=T)                  # 7 K' = 70
        sc["kf74"] = S.scene(35, 74, window=3, loop=2, n_mp=T + 1)              # 7 K' = 511 = T - 1: the last size below T
        sc["kf75"] = S.scene(36, 75, window=3, loop=2, n_mp=5)                  # 7 K' = 518: the first above T
        sc["edges17"] = S.scene(37, 18, window=1, loop=0, n_mp=3)               # 17 edges: 29 x 17 = 493 error elements, below T
        sc["edges18"] = S.scene(38, 19, window=1, loop=0, n_mp=3)               # 18 edges: 522, the first count above T (29 does not divide T, so no count equals it;
        #                                                                         the update phase of kf75 has 74 x 7 = 518 and its substitutions every length up to 517, T among them)
        for k, v in S.structures().items():                                     # chain, window 10, window 10 + loop 5: 11, 85 and 116 edges, the last two above 4 T error elements
            sc[k] = v
        sc["isolated"] = S.scene(39, 9, window=3, loop=2, n_mp=8, isolated=True)
        sc["scaled"] = S.scene(40, 12, window=3, loop=3, n_mp=9, cur_scale=0.9)
        sc["past_grid"] = S.scene(41, 6, window=2, loop=1, n_mp=FULL_GRID + 1)
        for n in (PT - 1, PT, PT + 1):                                          # around a block of k_ess_points
            sc["points%d" % n] = S.scene(42 + n, 5, window=2, loop=1, n_mp=n)
        sc["free_scale_long"] = S.free_scale_long()                             # 13 iterations without fix_scale
        _cache["scenes"] = sc
    return _cache["scenes"]


def _host(items, fix_scale):
    import essgraph_scene as S
    key = (tuple(id(i) for i in items), fix_scale)
    if key not in _cache:
        _cache[key] = S.HostEss().OptimizeEssentialGraph(items, fix_scale)
    return _cache[key]


def test_the_parity_scenes_are_well_conditioned_on_the_host():
    """no failed factorisation and at least 2 iterations in every parity scene; the sizes are the ones the docstrings name"""
    sc = _scenes()
    assert [len(sc[k]["edge_i"]) for k in ("edges17", "edges18")] == [17, 18] and len(sc["window_loop5"]["edge_i"]) * 29 > 4 * T and len(sc["window10"]["edge_i"]) * 29 > 4 * T
    for fs in (True, False):
        for name, it in sc.items():
            r = _host([it], fs)[0]
            assert r["solver_fail"] == 0 and r["n_iters"] >= 2 and r["n_active"] == len(it["kf_id"]) - 1 - (name == "isolated"), (name, fs, r["n_iters"], r["solver_fail"])


@pytest.mark.parametrize("fix_scale", [True, False])
def test_device_equals_the_host_twin_bit_for_bit(fix_scale):
    import essgraph_scene as S
    sc = _scenes(); names = list(sc)
    mt = _matcher(4)
    for at in range(0, len(names), 4):                                          # batches of mixed sizes, in the scenes' order
        group = names[at:at + 4]
        got = mt.OptimizeEssentialGraph([sc[k] for k in group], fix_scale)
        for k, g in zip(group, got):
            S.assert_same(g, _host([sc[k]], fix_scale)[0], (k, fix_scale))
    mt.close()


def test_items_of_a_batch_are_independent_and_the_workspace_may_grow():
    import essgraph_scene as S
    sc = _scenes()
    small, big, mid = sc["kf3"], sc["window_loop5"], sc["kf11"]
    mt = _matcher(4)
    alone = mt.OptimizeEssentialGraph([small], True)[0]
    S.assert_same(alone, _host([small], True)[0], "alone")
    for order in ([small, big, mid], [big, small, mid, small], [mid, big, small]):
        got = mt.OptimizeEssentialGraph(order, True)
        for it, g in zip(order, got):
            S.assert_same(g, _host([it], True)[0], "in a batch")
    S.assert_same(mt.OptimizeEssentialGraph([sc["kf75"]], True)[0], _host([sc["kf75"]], True)[0], "a larger call")       # the workspace grows
    S.assert_same(mt.OptimizeEssentialGraph([small], True)[0], alone, "a small call after a large one")
    mt.close()


def test_a_failed_factorisation_and_the_empty_cases_equal_the_host():
    import essgraph_scene as S
    f = S.failing_item()
    empty = S.copy_item(_scenes()["kf10"], edge_i=np.zeros(0, np.int32), edge_j=np.zeros(0, np.int32), edge_kind=np.zeros(0, np.uint8))
    nomp = S.copy_item(_scenes()["kf10"], x3Dw=np.zeros((0, 3), np.float32), mp_ref=np.zeros(0, np.int32))
    mt = _matcher(4)
    assert mt.OptimizeEssentialGraph([], True) == []
    for fs in (True, False):
        ref = S.HostEss().OptimizeEssentialGraph([f, empty, nomp, S.exact_item()], fs)
        assert ref[0]["solver_fail"] == 1 and ref[0]["n_iters"] == 1 and ref[1]["n_iters"] == -1 and ref[1]["n_active"] == 0
        got = mt.OptimizeEssentialGraph([f, empty, nomp, S.exact_item()], fs)
        for g, r, what in zip(got, ref, ("failing", "no edges", "no points", "exact")):
            S.assert_same(g, r, (what, fs))
    mt.close()


def test_on_a_handle_shared_with_the_other_solver_calls():
    """the call interleaved with local BA on one handle, with batches of changing order, each against its own host twin"""
    import essgraph_scene as S
    import localba_scene as LB
    sc = _scenes()
    mt = _matcher(2)
    lb = LB.scene(3, 3, 1, 20, kind="mixed", outliers=2)
    K = np.array([520.0, 516.0, 320.0, 240.0, 40.0], np.float32)
    lb_ref = LB.HostBA().LocalBundleAdjustment([lb], K=K)[0]
    first = mt.OptimizeEssentialGraph([sc["kf10"], sc["kf3"]], True)
    LB.assert_same(mt.LocalBundleAdjustment([lb])[0], lb_ref, "local BA after the essential graph")
    again = mt.OptimizeEssentialGraph([sc["kf3"], sc["kf10"]], True)
    for g, k in ((first[0], "kf10"), (first[1], "kf3"), (again[0], "kf3"), (again[1], "kf10")):
        S.assert_same(g, _host([sc[k]], True)[0], k)
    LB.assert_same(mt.LocalBundleAdjustment([lb])[0], lb_ref, "local BA once more")
    mt.close()


def test_error_paths_and_limits_return_the_host_codes_and_touch_nothing():
    import essgraph_scene as S
    from sindslam_amd._lib import lib
    from sindslam_amd.matcher import essgraph_items
    mt = _matcher(2)
    good = _scenes()["kf3"]
    six = S.scene(33, 6, 3, 2, 7)
    cases = [(it, SIND_E_ARG, 0) for it in S.bad_items().values()] + [(six, SIND_E_ARG, how) for how in S.TWEAKS.values()] + [(it, SIND_E_CAPACITY, 0) for it in S.capacity_items().values()]
    for it, code, how in cases:
        for items in ([it], [good, it]):
            arr, keep = essgraph_items(items)
            S.tweak(arr[len(items) - 1], how)
            for a in keep:
                a["Siw_out"][:] = 7.0; a["Tiw_out"][:] = 7.0; a["x3Dw_out"][:] = 7.0; a["n_iters"][:] = 77
            assert lib().sind_match_essential_graph(mt._h, arr, len(items), 1) == code
            assert S.host().sindh_essential_graph(arr, len(items), 1) == code
            for a in keep:
                assert (a["Siw_out"] == 7.0).all() and (a["Tiw_out"] == 7.0).all() and (a["x3Dw_out"] == 7.0).all() and a["n_iters"][0] == 77
    arr, keep = essgraph_items([good, good, good])
    assert lib().sind_match_essential_graph(mt._h, arr, 3, 1) == SIND_E_CAPACITY                 # B over max_batch
    assert lib().sind_match_essential_graph(mt._h, None, 1, 1) == SIND_E_ARG
    S.assert_same(mt.OptimizeEssentialGraph([good], True)[0], _host([good], True)[0], "after the refusals")
    mt.close()


def test_correct_loop_end_to_end_equals_the_host_library_run():
    """optimizer.correct_loop on the toy map, once over the device call and once over the host library: the same collected item, the same result bits, the same map"""
    import copy
    import essgraph_scene as S
    from sindslam_amd import optimizer as OPT
    kfs, mps, cur, loop, Scw, matched, _ = S.toy_map()
    kfs_h, mps_h = copy.deepcopy(kfs), copy.deepcopy(mps)
    mt = _matcher(1)
    tr, tr_h = {}, {}
    r = OPT.correct_loop(mt, kfs, mps, cur, loop, Scw, matched, True, trace=tr)
    r_h = OPT.correct_loop(S.HostEss(), kfs_h, mps_h, cur, loop, Scw, matched, True, trace=tr_h)
    mt.close()
    assert all(np.array_equal(tr["item"][k], tr_h["item"][k]) for k in tr["item"]) and r_h["n_iters"] >= 2 and r_h["solver_fail"] == 0
    S.assert_same(r, r_h, "correct_loop")
    assert all(np.array_equal(kfs[k]["Tcw"], kfs_h[k]["Tcw"]) for k in kfs) and all(np.array_equal(mps[m]["x3Dw"], mps_h[m]["x3Dw"]) for m in mps)
