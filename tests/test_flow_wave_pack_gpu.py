"""GPU: k_sor_wave with its column strips cut over groups of images laid side by side (FlowStage.set_wave_pack) against k_sor_color (solver mode 0) on the same inputs, bit
for bit.  Every batch entry has its own images and its own initial flow: an image that leaked into its neighbour in the virtual row would show."""
import functools

import numpy as np
import pytest

import flow_scene as S
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fs():
    from sindslam_amd.flow import FlowStage
    f = FlowStage(132, 98, max_batch=81)          # every level below is at most 132 x 98 pixels and more than 8192
    yield f
    f.close()


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@functools.lru_cache(maxsize=None)
def batch(w, h, B):
    """B different textured pairs (different shifts too) with B different initial flows; shared, never written"""
    rng = np.random.default_rng(1000 * w + h)
    pairs = [S.textured(w, h, 31 * w + h + 7 * b, dx=1 + b % 4, dy=-2 + b % 3) for b in range(B)]
    i0 = np.stack([p[0] for p in pairs]); i1 = np.stack([p[1] for p in pairs])
    u0 = rng.normal(0, 1.0, (B, h, w)).astype(np.float32); v0 = rng.normal(0, 1.0, (B, h, w)).astype(np.float32)
    for p in (i0, i1, u0, v0):
        p.setflags(write=False)
    return i0, i1, u0, v0


def solve(fs, args, mode, group=0, bands=0):
    try:
        fs.set_sor_variant(mode, 5, 64, 64); fs.set_wave_solver(True, 0, bands); fs.set_wave_pack(group)
        return fs.varref_f32(*args)
    finally:
        fs.set_sor_variant(); fs.set_wave_solver(); fs.set_wave_pack()


# (w, h, images, group, row bands, oracle too)
SHAPES = [(37, 230, 5, 3, 1, True),       # odd width, one gap column, three images in one wave, short last group
          (36, 240, 4, 3, 2, True),       # even width, a whole gap lane
          (61, 140, 5, 2, 1, False),      # two images in one wave
          (100, 90, 7, 3, 2, False),      # cuts inside images, next to seams
          (129, 67, 3, 3, 1, False),      # packed multi-strip
          (127, 66, 4, 2, 3, False),
          (230, 40, 5, 5, 1, False),
          (385, 24, 3, 3, 2, False)]      # a level lower than two halos


@pytest.mark.parametrize("w,h,B,group,bands,oracle", SHAPES)
def test_packed_wave_solver_equals_the_per_colour_kernel(fs, w, h, B, group, bands, oracle):
    """2 fixed-point iterations x 10 SOR iterations (5 x 25 where the oracle is asked too) with DeepFlow's level parameters: every float of u and v of every image"""
    assert w * h > 8192
    i0, i1, u0, v0 = batch(w, h, B)
    a, d, g, om = S.DEEPFLOW_LEVEL
    fp, sor = (5, 25) if oracle else (2, 10)
    args = (i0, i1, u0, v0, fp, sor, a, d, g, om)
    ru, rv = solve(fs, args, 0)
    gu, gv = solve(fs, args, 6, group, bands)
    for b in range(B):
        assert bits_equal(gu[b], ru[b]) and bits_equal(gv[b], rv[b]), (w, h, B, group, bands, b, int((gu[b] != ru[b]).sum()), int((gv[b] != rv[b]).sum()))
    if oracle:
        for b in range(B):
            ou, ov = O.varref(i0[b], i1[b], u0[b], v0[b], fp, sor, a, d, g, om)
            assert bits_equal(gu[b], ou) and bits_equal(gv[b], ov), (w, h, b, float(np.abs(gu[b] - ou).max()), float(np.abs(gv[b] - ov).max()))


def test_the_pipelines_path_and_the_switch(fs):
    """132 x 98 at 81 images with the automatic group and automatic bands (a launch of the batched pipeline), and the same with every image on its own: both the
    per-colour kernel's bits"""
    from sindslam_amd._lib import lib
    import ctypes as C
    out = (C.c_int * 6)()
    assert lib().sind_flow_wave_pack_layout(132, 98, 81, 0, 0, 0, out) == 0 and out[0] > 1, tuple(out)          # the automatic rule does pack this launch
    a, d, g, om = S.DEEPFLOW_LEVEL
    args = batch(132, 98, 81) + (2, 10, a, d, g, om)
    ru, rv = solve(fs, args, 0)
    gu, gv = solve(fs, args, 6, 0, 0)
    su, sv = solve(fs, args, 6, 1, 0)
    bad = [b for b in range(81) if not (bits_equal(gu[b], ru[b]) and bits_equal(gv[b], rv[b]))]
    assert not bad, ("packed", bad)
    assert bits_equal(su, ru) and bits_equal(sv, rv), "every image on its own"


def test_a_sparse_image_beside_a_textured_one(fs):
    """groups of two at 300 x 33: a sparse strip (tests/flow_scene.py: its increment falls through 2^-105 and the denormals, which sends its waves to the run with the IEEE
    division) left and right of a textured neighbour with an N(0, 1) flow; 1 x 100 iterations from the scene list.  The sparse images also equal the oracle."""
    seed, w, h, cw, fp, sor = S.SPARSE_SOLVER_SCENES[0]
    s0, s1 = S.sparse_strip(seed, w, h, cw)
    (t0, t1, tu, tv) = batch(w, h, 2)
    z = np.zeros((h, w), np.float32)
    a, d, g, om = S.DEEPFLOW_LEVEL
    args = (np.stack([s0, t0[0], t0[1], s0]), np.stack([s1, t1[0], t1[1], s1]), np.stack([z, tu[0], tu[1], z]), np.stack([z, tv[0], tv[1], z]), fp, sor, a, d, g, om)
    ru, rv = solve(fs, args, 0)
    gu, gv = solve(fs, args, 6, 2, 1)
    for b in range(4):
        assert bits_equal(gu[b], ru[b]) and bits_equal(gv[b], rv[b]), (b, int((gu[b] != ru[b]).sum()), int((gv[b] != rv[b]).sum()))
    ou, ov = O.varref(s0, s1, z, z, fp, sor, a, d, g, om)
    assert S.count_tiny(ou)[0] > 0                                              # the scene does reach the range below 2^-116
    for b in (0, 3):
        assert bits_equal(gu[b], ou) and bits_equal(gv[b], ov), b
