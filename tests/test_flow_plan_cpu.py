"""CPU: which kernel solves a flow level (sind_flow_sor_plan: sor_plan of flow_sor.hip, host arithmetic only).  The policy as it stood before it became one function is
restated here in Python, from the launch code it was buried in, and compared with the library over a grid of levels, batch sizes and settings; then the properties of a
plan, and the claims the GPU tests make in their comments about the kernel their shapes reach."""
import ctypes as C
import itertools

import pytest

import flow_scene as S
import oracle_lib as O

CHAIN, COLOR, TILES, ONE_WG, WAVE, STREAM, FUSED = range(7)
E_ARG = -1


def plan(w, h, B, total, mode=4, fuse=5, tw=64, th=64, wave=1, min_b=80, lat=1, chain=1, cap=130):
    """(kernel, [iterations per launch]) or None where the library says SIND_E_ARG"""
    from sindslam_amd._lib import lib
    out = (C.c_int * cap)()
    rc = lib().sind_flow_sor_plan(mode, fuse, tw, th, wave, min_b, lat, chain, w, h, B, total, out, cap)
    if rc != 0:
        assert rc == E_ARG, rc
        return None
    return out[0], list(out[2:2 + out[1]])


# ---- the policy, restated: varref_level's chain test, then sor_iterations' cascade, with the constants of the kernels' files ----------------------------------------------
def divup(a, b):
    return -(-a // b)


def chain_strip(w, h):                      # flow_coarse.hip: strip half-width (1 or 2) at which 1024 threads and 64 floats per LDS row hold the level, else 0
    for P in (1, 2):
        SW = divup(w, 2 * P)
        if 2 * divup(SW * ((h + 1) // 2), 64) * 64 <= 1024 and P * SW + P + 1 <= 64:
            return P
    return 0


def tile_count(w, h, k):                    # k_sor_tile: 64-pixel tiles keep 64 - 4 k pixels per edge
    keep = 64 - 4 * k
    return 1 << 30 if keep < 4 else divup(w, keep) * divup(h, keep)


def latency_plan(w, h, B, total):           # the fewest launches (at most 13 iterations each) whose tiles all find one of 256 compute units
    for n in range(1, total + 1):
        base, rem = divmod(total, n)
        kmax = base + (1 if rem else 0)
        if kmax > 13:
            continue
        if tile_count(w, h, kmax) * B > 256:
            if kmax <= 5:
                break
            continue
        return [base + 1] * rem + [base] * (n - rem)
    return []


def fused_threads(EW, EH):
    return 2 * divup((EW // 8) * ((EH + 1) // 2), 64) * 64


def fused_lds(EW, nt):
    rows = 2 * ((nt // 2) // (EW // 8))
    stride = (EW // 8 + 2) + (4 - (EW // 8 + 2)) % 8
    return 6 * (rows + 2) * stride * 16


def policy(w, h, B, total, mode, wave, lat, chain, fuse=5, tw=64, th=64, min_b=80, eps=0.001):
    if chain and eps >= 1e-12 and mode != 0 and chain_strip(w, h):
        return CHAIN, [total]
    if mode == 0:
        return COLOR, [1] * total
    EW = divup(w, 8) * 8
    if lat and mode == 4:
        p = latency_plan(w, h, B, total)
        if p and not (len(p) > 1 and fused_threads(EW, h) <= 512):
            return TILES, p
    if fused_threads(EW, h) <= 1024:
        return (ONE_WG, [total]) if fused_lds(EW, fused_threads(EW, h)) <= 150 * 1024 else None
    if total % 5 == 0 and (mode == 6 or (mode == 4 and wave and B >= min_b)):
        return WAVE, [5] * (total // 5)
    if h >= 4 and total % 5 == 0 and (mode == 5 or (mode == 4 and B >= min_b)):
        return STREAM, [5] * (total // 5)
    nt = fused_threads(tw, th)
    if nt > 1024 or 4 * fuse >= min(tw, th) or fused_lds(tw, nt) > 150 * 1024:
        return None
    return FUSED, [fuse] * (total // fuse) + ([total % fuse] if total % fuse else [])


def grid_sizes():
    sizes = set()
    for w, h in [(384, 288), (640, 480), (1280, 720), (768, 432)]:
        sizes.update(O.deepflow_levels(w, h))
    # both sides of 4 096 pixels (the chain's limit, the 512-thread one-workgroup kernel) and of 8 192 (the 1024-thread one)
    sizes.update([(64, 64), (65, 63), (64, 65), (63, 64), (91, 45), (90, 45), (92, 45), (120, 34), (124, 33), (128, 64), (128, 63), (128, 65), (129, 64), (127, 64), (100, 81),
                  (100, 82), (104, 78), (26, 78), (8, 6), (5, 7), (1000, 9), (1001, 8), (16, 600), (9, 3)])
    return sorted(sizes)


def test_plan_equals_the_policy_restated():
    sizes = grid_sizes()
    assert len(sizes) > 150
    bad = []
    for (w, h), B, mode, wave, lat, chain, total in itertools.product(sizes, (1, 2, 3, 8, 79, 80, 170, 512), (0, 4, 5, 6), (0, 1), (0, 1), (0, 1), (5, 25, 7)):
        got, want = plan(w, h, B, total, mode=mode, wave=wave, lat=lat, chain=chain), policy(w, h, B, total, mode, wave, lat, chain)
        if got != want:
            bad.append(((w, h, B, total, mode, wave, lat, chain), got, want))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("fuse,tw,th", [(1, 64, 64), (3, 32, 32), (12, 64, 64), (7, 128, 64), (2, 16, 64), (2, 16, 512)])
def test_plan_equals_the_policy_on_other_tiles(fuse, tw, th):
    """the tiled kernel's own settings, at batch sizes that take it (latency tiles off); 16 x 512 tiles pass the setter and exceed the LDS: an error in both"""
    for (w, h), B, total in itertools.product([(129, 67), (384, 288), (768, 432), (303, 65)], (1, 79, 170), (5, 25, 7)):
        for mode in (4, 5, 6):
            assert plan(w, h, B, total, mode=mode, fuse=fuse, tw=tw, th=th, lat=0, wave=0) == policy(w, h, B, total, mode, 0, 0, 1, fuse=fuse, tw=tw, th=th), (w, h, B, total, mode)


def test_plan_properties():
    for (w, h), B, mode, wave, lat, total in itertools.product(grid_sizes()[::3], (1, 3, 80, 512), (0, 4, 5, 6), (0, 1), (0, 1), (5, 25, 7)):
        p = plan(w, h, B, total, mode=mode, wave=wave, lat=lat)
        if p is None:
            continue
        kernel, iters = p
        what = (w, h, B, total, mode, wave, lat, p)
        assert sum(iters) == total and all(k >= 1 for k in iters), what
        if kernel == TILES:
            assert mode == 4 and lat and max(iters) <= 13 and tile_count(w, h, max(iters)) * B <= 256, what
        if kernel in (WAVE, STREAM):
            assert total % 5 == 0 and set(iters) == {5}, what
        if mode == 0:
            assert kernel == COLOR and iters == [1] * total, what
        if kernel in (CHAIN, ONE_WG):
            assert iters == [total], what


def test_gpu_test_shapes_reach_the_kernels_their_comments_name():
    import test_flow_coarse_gpu as TC
    import test_flow_gpu as TF
    import test_flow_sparse_gpu as TS
    # test_flow_gpu.py: two images, 25 iterations; mode 5 runs k_sor_stream on every STREAM_SHAPES size, mode 6 k_sor_wave on every WAVE_SHAPES size
    for w, h in TF.STREAM_SHAPES:
        assert plan(w, h, 2, 25, mode=5) == (STREAM, [5] * 5), (w, h)
    for w, h, _bands in TF.WAVE_SHAPES:
        assert plan(w, h, 2, 25, mode=6) == (WAVE, [5] * 5), (w, h)
    # test_flow_coarse_gpu.py: the handle's defaults; the k_sor_tile list covers the four plans its comment names, and every pyramid level of at most 4 096 pixels is the chain's
    plans = {(w, h, B): plan(w, h, B, 25) for w, h, B in TC.TILE_SHAPES}
    assert all(p is not None and p[0] == TILES for p in plans.values()), plans
    assert {tuple(p[1]) for p in plans.values()} == {(13, 12), (9, 8, 8), (7, 6, 6, 6), (5, 5, 5, 5, 5)}, plans
    for w, h in TC.chain_levels(384, 288) + TC.chain_levels(768, 432):
        assert plan(w, h, 1, 25) == (CHAIN, [25]) and plan(w, h, 3, 25) == (CHAIN, [25]), (w, h)
        assert plan(w, h, 1, 25, chain=0)[0] != CHAIN, (w, h)
    # test_flow_sparse_gpu.py: two images; the rows of the solver table, the k_sor_tile scenes and the chain scenes
    named = {"color": COLOR, "fused": FUSED, "stream": STREAM, "wave1": WAVE, "wave2": WAVE}
    assert sorted(named) == sorted(s[0] for s in TS.SOLVERS)
    for (_seed, w, h, _cw, _fp, sor), (name, mode, tiles, _bands) in itertools.product(S.SPARSE_SOLVER_SCENES, TS.SOLVERS):
        assert plan(w, h, 2, sor, mode=mode, lat=int(tiles))[0] == named[name], (w, h, sor, name)
    for _seed, w, h, _cw, _fp, sor in S.SPARSE_TILE_SCENES:
        assert plan(w, h, 2, sor)[0] == TILES, (w, h, sor)
    for _seed, w, h, _cw, _fp, sor in S.SPARSE_CHAIN_SCENES:
        assert plan(w, h, 2, sor)[0] == CHAIN, (w, h, sor)


def test_bad_arguments():
    from sindslam_amd._lib import lib
    out = (C.c_int * 32)()
    ok = dict(mode=4, fuse=5, tw=64, th=64, wave=1, min_b=80, lat=1, chain=1, w=384, h=288, B=2, total=25)

    def rc(out_=out, cap=32, **kw):
        a = dict(ok, **kw)
        return lib().sind_flow_sor_plan(a["mode"], a["fuse"], a["tw"], a["th"], a["wave"], a["min_b"], a["lat"], a["chain"], a["w"], a["h"], a["B"], a["total"], out_, cap)
    assert rc() == 0
    assert rc(out_=None) == E_ARG
    assert rc(w=0) == E_ARG and rc(h=0) == E_ARG and rc(B=0) == E_ARG and rc(total=0) == E_ARG and rc(min_b=0) == E_ARG
    assert rc(mode=1) == E_ARG and rc(mode=7) == E_ARG and rc(mode=-1) == E_ARG
    # tiles sind_flow_set_sor_tiled rejects: width not a multiple of 8, odd height, threads not a multiple of 128 or above 1024, a halo that leaves nothing
    for fuse, tw, th in [(5, 60, 64), (5, 64, 63), (5, 24, 24), (5, 128, 128), (0, 64, 64), (13, 64, 64), (8, 32, 32), (5, 8, 128)]:
        assert rc(fuse=fuse, tw=tw, th=th) == E_ARG, (fuse, tw, th)
    assert rc(mode=0, cap=26) == E_ARG and rc(mode=0, cap=27) == 0         # 25 launches need 27 words
    assert len(lib().sind_last_error()) > 0
