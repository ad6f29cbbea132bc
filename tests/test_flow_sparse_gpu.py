"""GPU parity of the dense-flow path on sparse, flat, static and saturated content, bit for bit against the CPU oracle.

Every other flow test feeds the kernels a band-limited random texture and an initial flow drawn from N(0, 1).  Here the solvers meet exact zeros, values below 2^-100,
denormals (the increment that spreads from a textured strip into a flat field: tests/flow_scene.py, and tests/test_flow_sparse_cpu.py for what the oracle reaches there),
saturated plateaus, rounding ties of the warp and positions outside the frame.  Solver mode 0 (k_sor_color, the compiler's IEEE division) is the control of the solver
kernels that divide through a reciprocal."""
import ctypes as C
import functools

import numpy as np
import pytest

import flow_scene as S
import oracle_lib as O
from sindslam_amd.synth import TUM3

pytestmark = pytest.mark.gpu
K3 = (TUM3["fx"], TUM3["fy"], TUM3["cx"], TUM3["cy"], TUM3["depth_factor"])


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def diff_report(g, o):
    """differing pixels, those of them with an oracle value of at least 2^-100, and the largest difference"""
    bad = g.view(np.uint32) != o.view(np.uint32)
    return int(bad.sum()), int((bad & (np.abs(o) >= 2.0 ** -100)).sum()), float(np.abs(g.astype(np.float64) - o).max())


@pytest.fixture(scope="module")
def fs_big():
    from sindslam_amd.flow import FlowStage
    f = FlowStage(768, 432, max_batch=2)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fs():
    from sindslam_amd.flow import FlowStage
    f = FlowStage(384, 288, max_batch=2)
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def sparse_case(scene):
    """(i0, i1, zero flow, oracle u, oracle v) of a sparse scene: computed once, shared by every kernel's test, never written"""
    seed, w, h, cw, fp, sor = scene
    i0, i1 = S.sparse_strip(seed, w, h, cw)
    z = np.zeros((h, w), np.float32)
    a, d, g, om = S.DEEPFLOW_LEVEL
    ou, ov = O.varref(i0, i1, z, z, fp, sor, a, d, g, om)
    for p in (i0, i1, z, ou, ov):
        p.setflags(write=False)
    return i0, i1, z, ou, ov


def solve_sparse(f, scene):
    i0, i1, z, ou, ov = sparse_case(scene)
    a, d, g, om = S.DEEPFLOW_LEVEL
    gu, gv = f.varref_f32(np.stack([i0, i0]), np.stack([i1, i1]), np.stack([z, z]), np.stack([z, z]), scene[4], scene[5], a, d, g, om)
    return gu, gv, ou, ov


def assert_equals_oracle(gu, gv, ou, ov, what):
    for b in range(gu.shape[0]):
        assert bits_equal(gu[b], ou), (what, "u", b) + diff_report(gu[b], ou)
        assert bits_equal(gv[b], ov), (what, "v", b) + diff_report(gv[b], ov)


# (name, solver mode, latency tiles, row bands of the one-wave solver): k_sor_color, k_sor_fused on 64 x 64 tiles, k_sor_stream, k_sor_wave in one band and in two
SOLVERS = [("color", 0, False, 0), ("fused", 4, False, 0), ("stream", 5, False, 0), ("wave1", 6, False, 1), ("wave2", 6, False, 2)]


@pytest.mark.parametrize("coef", [0, 1, 2])
@pytest.mark.parametrize("solver", SOLVERS, ids=[s[0] for s in SOLVERS])
@pytest.mark.parametrize("scene", S.SPARSE_SOLVER_SCENES, ids=lambda s: "seed%d_%dx%d_%dx%d" % (s[0], s[1], s[2], s[4], s[5]))
def test_solvers_on_sparse_strips_equal_the_oracle(fs_big, scene, solver, coef):
    """zero initial flow, DeepFlow's level parameters: the increment decays from the textured strip through 2^-105, the denormals and exact zeros inside ONE launch's
    working set; every solver kernel and every coefficient kernel returns the oracle's bits"""
    name, mode, tiles, bands = solver
    try:
        fs_big.set_sor_variant(mode, 5, 64, 64); fs_big.set_latency_tiles(tiles); fs_big.set_wave_solver(True, 0, bands); fs_big.set_coef_kernel(coef)
        gu, gv, ou, ov = solve_sparse(fs_big, scene)
    finally:
        fs_big.set_sor_variant(); fs_big.set_latency_tiles(True); fs_big.set_wave_solver(); fs_big.set_coef_kernel(1)
    assert_equals_oracle(gu, gv, ou, ov, (scene, name, coef))


@pytest.mark.parametrize("scene", S.SPARSE_TILE_SCENES, ids=lambda s: "seed%d_%dx%d_%dx%d" % (s[0], s[1], s[2], s[4], s[5]))
def test_latency_tiles_on_sparse_strips_equal_the_oracle(fs, scene):
    """k_sor_tile (the handle's default at two images: 1024-thread tiles, up to 13 iterations per launch)"""
    fs.set_latency_tiles(True)
    gu, gv, ou, ov = solve_sparse(fs, scene)
    assert_equals_oracle(gu, gv, ou, ov, (scene, "tile"))


@pytest.mark.parametrize("scene", S.SPARSE_CHAIN_SCENES, ids=lambda s: "seed%d_%dx%d_cw%d_%dx%d" % s)
def test_chain_on_sparse_strips_equals_the_oracle(fs, scene):
    """k_coarse_chain (one workgroup's level in one launch) and, with the chain off, the per-stage kernels on the same level (k_sor_fused as one workgroup)"""
    fs.set_coarse_chain(True)
    gu, gv, ou, ov = solve_sparse(fs, scene)
    try:
        fs.set_coarse_chain(False)
        su, sv, _, _ = solve_sparse(fs, scene)
    finally:
        fs.set_coarse_chain(True)
    assert_equals_oracle(gu, gv, ou, ov, (scene, "chain"))
    assert_equals_oracle(su, sv, ou, ov, (scene, "per-stage"))


PYRAMID_SCENES = {"flat128": lambda w, h: S.flat(128, w, h), "flat0": lambda w, h: S.flat(0, w, h), "flat255": lambda w, h: S.flat(255, w, h),
                  "static": lambda w, h: S.static_pair(w, h, 1), "blob": S.blob_on_flat, "plateau255": lambda w, h: S.plateau(w, h, 2, 255),
                  "plateau0": lambda w, h: S.plateau(w, h, 3, 0)}


@pytest.fixture(scope="module")
def pyramids():
    from sindslam_amd.flow import FlowStage
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = FlowStage(w, h, max_batch=2)
        return made[(w, h)]
    yield get
    for f in made.values():
        f.close()


@pytest.mark.parametrize("name", list(PYRAMID_SCENES))
@pytest.mark.parametrize("w,h", [(96, 72), (384, 288)])
def test_deepflow_on_flat_static_and_saturated_content_equals_the_oracle(pyramids, w, h, name):
    """whole pyramids (every level in the chain at 96 x 72; chain, tiles and level transitions at 384 x 288) on content with exact zeros everywhere or on one half"""
    a, b = PYRAMID_SCENES[name](w, h)
    f = pyramids(w, h)
    assert f.levels() == O.deepflow_levels(w, h)
    u, v = f.deepflow(np.stack([a, b]), np.stack([b, a]))
    of = O.deepflow(a, b); ob = of if name.startswith("flat") or name == "static" else O.deepflow(b, a)
    for k, o in enumerate((of, ob)):
        assert bits_equal(u[k], o[..., 0]), (w, h, name, k, "u") + diff_report(u[k], np.ascontiguousarray(o[..., 0]))
        assert bits_equal(v[k], o[..., 1]), (w, h, name, k, "v") + diff_report(v[k], np.ascontiguousarray(o[..., 1]))


@pytest.mark.parametrize("coef", [0, 1])
@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("w,h", [(97, 61), (129, 67)])
def test_warp_ties_and_out_of_frame_positions_equal_the_oracle(fs_big, w, h, mode, coef):
    """an initial flow of odd multiples of 1/64 up to +- 2 max(w, h): every warp coordinate times 32 is an exact .5 tie for cvRound and many positions lie outside the frame
    on each side (BORDER_REPLICATE); 3 fixed-point iterations re-enter the coefficients with the increment of such a field"""
    i0, i1 = S.textured(w, h, 11 * w + h)
    u0, v0 = S.tie_flow(w, h, w + h)
    a, d, g, om = S.DEEPFLOW_LEVEL
    ou, ov = tie_oracle(w, h)
    try:
        fs_big.set_sor_variant(mode, 5, 64, 64); fs_big.set_coef_kernel(coef)
        gu, gv = fs_big.varref_f32(np.stack([i0, i0]), np.stack([i1, i1]), np.stack([u0, u0]), np.stack([v0, v0]), 3, 10, a, d, g, om)
    finally:
        fs_big.set_sor_variant(); fs_big.set_coef_kernel(1)
    assert_equals_oracle(gu, gv, ou, ov, (w, h, mode, coef))


@functools.lru_cache(maxsize=None)
def tie_oracle(w, h):
    i0, i1 = S.textured(w, h, 11 * w + h)
    u0, v0 = S.tie_flow(w, h, w + h)
    a, d, g, om = S.DEEPFLOW_LEVEL
    ou, ov = O.varref(i0, i1, u0, v0, 3, 10, a, d, g, om)
    assert np.isfinite(ou).all() and np.isfinite(ov).all()
    ou.setflags(write=False); ov.setflags(write=False)
    return ou, ov


def dyna_content(name, frames):
    bgr, depth = frames
    if name == "static":
        return [bgr[0]] * 3, depth[0]
    if name == "flat":
        return [np.full_like(bgr[0], 128)] * 3, depth[0]
    sat = S.half_saturated(bgr[:3])
    return [sat[0], sat[1], sat[2]], depth[2]


@pytest.mark.parametrize("content", ["static", "flat", "half_saturated"])
def test_dynadetect_on_static_flat_and_half_saturated_frames_equals_the_oracle(frames, content):
    """three frames through DynaDetect at 640 x 480: every debug stage that tests/test_dyna_gpu.py compares and both outputs equal the oracle's; H and the thresholds as bit
    patterns (identical and flat frames give an identity with one -0 and thresholds 0, 0, 1, inf, inf; the large-motion flag is set at zero flow)"""
    from sindslam_amd.dyna import DynaDetect
    (f0, f1, f2), dep = dyna_content(content, frames)
    ref = O.DynaDetect(f1, f0, *K3); gpu = DynaDetect(f1, f0, *K3)
    try:
        rd, rl = ref.detect(f2, dep); r = ref.debug()
        gd, gl = gpu.DetectDynaArea(f2, dep, 2); g = gpu.debug()
    finally:
        gpu.close()
    ff = np.stack([r["flow_full"][..., 0], r["flow_full"][..., 1]])
    assert bits_equal(g["flow_full"], ff), diff_report(g["flow_full"], ff)
    assert g["info"][0] == r["info"][0], "largeMotion flag"
    assert g["info"][1] == r["info"][1]
    assert np.array_equal(g["H"].view(np.uint64), r["H"].view(np.uint64)), (g["H"], r["H"])
    assert np.array_equal(g["hist"], r["hist"])
    assert bits_equal(g["thr"], r["thr"]), (g["thr"], r["thr"])
    assert np.array_equal(g["mask_low"], r["mask_low"]) and np.array_equal(g["mask_high"], r["mask_high"])
    assert np.array_equal(g["total_area"], r["total_area"])
    assert np.array_equal(g["kmeans_label"], r["kmeans_label"])
    assert np.array_equal(g["centers"], r["centers"])
    assert np.array_equal(g["grad_edge"], r["grad_edge"]) and np.array_equal(g["plane_contours"], r["plane_contours"])
    assert np.array_equal(g["occ2"], r["occ2"]) and np.array_equal(g["occ1"], r["occ1"])
    assert g["info"][2] == r["info"][2], "number of pieces"
    assert np.array_equal(gd, rd) and np.array_equal(gl, rl)
    assert set(np.unique(gd)) <= {0, 125, 255}
    if content != "half_saturated":
        assert r["info"].tolist() == [1, 2961, 15] and np.signbit(r["H"][2, 1]) and np.isinf(r["thr"][3:]).all()
    else:
        assert r["info"][0] == 0 and np.count_nonzero(r["hist"]) > 100          # an ordinary frame on the left half


def test_quotients_below_the_exhaustive_scans_equal_the_ieee_division():
    """sor_div and kc_div against n / a where sind_debug_rcp_scan and sind_debug_coef_math_scan do not look: every divisor significand x the divisor exponents -7 .. 14 x a
    numerator per binary exponent from -149 (the smallest denormal) up to the divisor's exponent - 40, and the numerators +0 and -0: not one of 2 x 2.1e10 quotients differs"""
    from sindslam_amd._lib import check, lib
    counts = (C.c_ulonglong * 3)(); by_exp = (C.c_ulonglong * 124)(); max_exp = C.c_int(0)
    check(lib().sind_debug_div_scan(0, counts, C.byref(max_exp), by_exp), "sind_debug_div_scan")
    worst = {e - 149: int(n) for e, n in enumerate(by_exp) if n}
    print("sor_div:", counts[0], "kc_div:", counts[1], "zero numerators:", counts[2], "largest failing numerator exponent:", max_exp.value, "by exponent:", worst)
    assert counts[0] == 0 and counts[1] == 0 and counts[2] == 0 and max_exp.value == -1000, (counts[0], counts[1], counts[2], max_exp.value, worst)
    assert lib().sind_debug_div_scan(0, None, C.byref(max_exp), None) == -1
