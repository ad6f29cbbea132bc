"""CPU: the numpy references of depth_ref.py against the oracle on every scene of depth_scene.py, the conditions that keep the GPU tests of the depth half from
passing on empty outputs (from the oracle alone), and the proof that every tie scene really holds its tie."""
import functools

import numpy as np
import pytest

import depth_ref as R
import depth_scene as S
import oracle_lib as O


@functools.lru_cache(maxsize=None)
def _case(w, h, intr, base, kind):
    bgr, depth, K = S.stream_case(w, h, kind, intr, base)
    return depth, K, R.oracle_stages(bgr, depth, K)


def _nz(img):
    return int((img > 0).sum())


# ---------------------------------------------------------------- the references against the oracle
@pytest.mark.parametrize("w,h", S.FRONT_SIZES)
def test_sorted_median_equals_the_oracle_median(w, h):
    for name, (d, _) in S.front_frames(w, h).items():
        assert np.array_equal(R.median5(d).astype(np.float32), O.median5_f32(d.astype(np.float32))), name


@pytest.mark.parametrize("w,h", [(64, 64), (128, 72), (192, 136)])          # (the oracle's detector does not take 71 x 13)
def test_reference_chain_equals_the_oracle_on_the_front_frames(w, h):
    """median -> edge rule -> opening == the oracle's grad_edge, total_area == the oracle's, on every front frame (colour from the stream: it does not matter here)"""
    bgr, _, K = S.stream_case(w, h, "plain")
    for name, (d, ds) in S.front_frames(w, h).items():
        ref = O.DynaDetect(bgr[1], bgr[0], *K[:4], ds)
        ref.detect(bgr[2], d); r = ref.debug(); f = R.front(d, ds)
        assert np.array_equal(f["edge"], r["grad_edge"]), name
        assert np.array_equal(f["total_area"], r["total_area"]), name


@pytest.mark.parametrize("w,h,intr,base", S.CONTENT_SIZES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_reference_chain_equals_the_oracle_on_the_stream_scenes(w, h, intr, base, kind):
    depth, K, st = _case(w, h, intr, base, kind)
    for k, t in enumerate((2, 3)):
        f = R.front(depth[t], K[4])
        assert np.array_equal(f["filt"].astype(np.float32), O.median5_f32(depth[t].astype(np.float32)))
        assert np.array_equal(f["edge"], st[k]["grad_edge"]) and np.array_equal(f["total_area"], st[k]["total_area"]), (kind, t)


# ---------------------------------------------------------------- the GPU tests do not pass on empty outputs
@pytest.mark.parametrize("w,h,intr,base", S.CONTENT_SIZES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_stream_scenes_reach_every_stage(w, h, intr, base, kind):
    _, _, st = _case(w, h, intr, base, kind)
    for o in st:
        if kind in ("plain", "saturated", "steps", "border"):
            assert o["pieces"] >= 8, o["pieces"]
            assert _nz(o["occ2"]) > 0 and _nz(o["plane_contours"]) > 0 and _nz(o["grad_edge"]) > 0
            assert (o["dyna"] == 255).sum() > 0 and (o["dyna"] == 125).sum() > 0
        elif kind == "lowrange":
            assert _nz(o["grad_edge"]) == 0 and _nz(o["plane_contours"]) > 0
        else:                                  # speckle: at 192 px a plane may be lost to the speckle (too few 16 x 16 blocks stay whole)
            assert _nz(o["grad_edge"]) > 0
            if w >= 256:
                assert _nz(o["plane_contours"]) > 0
        print(w, h, kind, "pieces", o["pieces"], "edge", _nz(o["grad_edge"]), "planes", _nz(o["plane_contours"]), "occ2", _nz(o["occ2"]),
              "dynamic", int((o["dyna"] == 255).sum()), "static", int((o["dyna"] == 125).sum()))


def test_rewritten_depth_is_what_the_kinds_say():
    for (w, h, intr, base) in S.CONTENT_SIZES:
        bgr, plain, _ = S.stream_case(w, h, "plain", intr, base)
        d = S.stream_case(w, h, "speckle", intr, base)[1][2]; ch = d != plain[2]
        assert 0 < ch.sum() <= 0.003 * w * h and set(np.unique(d[ch])) <= {0, 65535} and (d[ch] == 0).any() and (d[ch] == 65535).any()
        assert (ch.reshape(h // 8, 8, w // 8, 8).sum((1, 3)) == 64).sum() == 0                    # single pixels, not 8 x 8 blocks
        d = S.stream_case(w, h, "saturated", intr, base)[1][2]
        assert (d == 65535).sum() >= w * h // 4 + 3 * w and (d[:3] == 65535).all() and (d[:, -3:] == 65535).all()
        d = S.stream_case(w, h, "lowrange", intr, base)[1][2]; assert d.max() == 510
        d = S.stream_case(w, h, "border", intr, base)[1][2]
        assert not d[:3].any() and not d[:, :3].any() and not d[-3:].any() and not d[:, -3:].any() and (d[3, 4:-4] == 60000).all() and (d[4:-4, 3] == 1).all()
        d = S.stream_case(w, h, "steps", intr, base)[1][2].astype(np.int64)
        assert d[0, 0] == base + 1 and d[1, 16] - d[1, 15] == 400 and d[16, 1] - d[15, 1] == 401 and d[7, 5] - d[7, 6] == 1


def test_small_plain_sizes_run_without_planes_or_dynamic_pixels():
    for (w, h) in S.SMALL_PLAIN:
        _, _, st = _case(w, h, "TUM3", 5000, "plain")
        for o in st:
            assert _nz(o["plane_contours"]) == 0 and (o["dyna"] == 255).sum() == 0 and _nz(o["grad_edge"]) > 0 and _nz(o["total_area"]) > 0


# ---------------------------------------------------------------- every tie scene holds its tie, in the reference's own filtered image
@pytest.mark.parametrize("w,h", S.FRONT_SIZES)
def test_tie_scenes_hold_their_ties(w, h):
    fr = S.front_frames(w, h)
    for name in ("ties_400", "ties_3pct", "half_even", "half_odd") + tuple(f"ramp_{ds:g}" for ds in S.SCALES_6M):
        assert np.array_equal(R.median5(fr[name][0]), fr[name][0]), name + ": not a fixed point of the median"
    r = R.front(*fr["ties_400"])["rule"]; v = set(np.unique(r["val_max"]).tolist())
    assert {400.0, 401.0} <= v and _nz(R.front(*fr["ties_400"])["edge_pre"]) > 0
    assert not r["edge"][3:-3, 3:-3][r["val_max"] == 400].any() and r["edge"][3:-3, 3:-3][r["val_max"] == 401].all()
    r = R.front(*fr["ties_3pct"])["rule"]; at = r["depth1"] == 20000
    assert {600.0, 601.0} <= set(np.unique(r["val_max"][at]).tolist()) and np.float32(20000) * np.float32(0.03) == np.float32(600)
    assert not r["edge"][3:-3, 3:-3][at & (r["val_max"] == 600)].any() and r["edge"][3:-3, 3:-3][at & (r["val_max"] == 601)].all()
    r = R.front(*fr["half_even"])["rule"]; assert r["depth_max"] == 40000 and {0.0, 1.0} <= set(r["half_margin"].tolist())
    r = R.front(*fr["half_odd"])["rule"]; assert r["depth_max"] == 40001 and {-0.5, 0.5} <= set(r["half_margin"].tolist())
    for ds in S.SCALES_6M:
        r = R.front(*fr[f"ramp_{ds:g}"])["rule"]; q = r["quotient"]
        assert (q < 6).any() and (q >= 6).any() and 0 < _nz(r["total_area"]) < (h - 6) * (w - 6), ds
        # the two raw values next to the limit are both in the frame: the largest valid one and its successor
        d1 = r["depth1"]; assert d1[q < 6].max() + 1 == d1[q >= 6].min()
    p = R.depth_norm_products(fr["norm_510"][0]); assert ((p - np.floor(p)) == 0.5).sum() > 0
    assert np.array_equal(R.depth_norm(fr["norm_510"][0])[fr["norm_510"][0] % 2 == 1] % 2, np.zeros((fr["norm_510"][0] % 2 == 1).sum(), np.uint8))      # ties go to the even value
    assert fr["norm_65535"][0].max() == 65535 and fr["norm_1"][0].max() == 1 and fr["zero"][0].max() == 0


@pytest.mark.parametrize("w,h", S.FRONT_SIZES)
def test_median_and_maxima_scenes(w, h):
    fr = S.front_frames(w, h)
    d = fr["salt_pepper"][0]; noise = np.isin(d, [0, 1, 32768, 65535])
    assert 0.25 < noise.mean() < 0.36 and noise[0, 0] and noise[0, -1] and noise[-1, 0] and noise[-1, -1]
    assert noise[0].any() and noise[-1].any() and noise[:, 0].any() and noise[:, -1].any()
    f = R.front(d, 5000.0); assert f["max_raw"] == 65535 and (f["filt"] != d).mean() > 0.25
    for name, pos in (("max_first", 0), ("max_last", w * h - 1)):
        d = fr[name][0]; f = R.front(d, 5000.0)
        assert np.flatnonzero(d == d.max()).tolist() == [pos] and f["max_raw"] == 50001
        assert np.flatnonzero(f["filt"] == f["filt"].max()).tolist() == [pos] and f["max_filt"] == 50000
    for names, ds in S.front_batches(w, h):
        assert len({fr[n][0].tobytes() for n in names}) == 3 and len({int(fr[n][0].max()) for n in names}) == 3, names
    lk = S.rewrite("lowrange", np.arange(w * h, dtype=np.uint16).reshape(h, w) * 7 + 3); p = R.depth_norm_products(lk)
    assert lk.max() == 510 and ((p - np.floor(p)) == 0.5).sum() > 0


# ---------------------------------------------------------------- the scenes tell a rule that is off by one rounding from the reference's
def _edge_rule_variant(filt, depth_scale, variant):
    """the edge rule of depth_ref.edge_rule with ONE comparison or rounding changed"""
    F = np.float32; f = np.asarray(filt).astype(F); h, w = f.shape
    half = F(F(f.max()) * F(0.5)); d1 = f[3:h - 3, 3:w - 3]
    q = d1 * (F(1) / F(depth_scale)) if variant == "reciprocal" else d1.astype(np.float64) / float(F(depth_scale)) if variant == "fp64" else d1 / F(depth_scale)
    total = (d1 > 0) & (q < F(6)); val_max = np.zeros_like(d1)
    for i in range(-2, 3):
        for j in range(-2, 3):
            diff = d1 - f[3 + i:h - 3 + i, 3 + j:w - 3 + j]
            skip = diff >= half if variant == "half_ge" else diff > half
            val_max = np.where(skip, val_max, np.maximum(val_max, np.abs(diff)))
    e = ((val_max >= d1 * F(0.03)) if variant == "pct_ge" else (val_max > d1 * F(0.03))) & ((val_max >= F(400)) if variant == "400_ge" else (val_max > F(400)))
    return e, total


@pytest.mark.parametrize("w,h", S.FRONT_SIZES)
def test_scenes_tell_a_changed_rule_apart(w, h):
    fr = S.front_frames(w, h)

    def differs(name, variant):
        d, ds = fr[name]; r = R.edge_rule(d, ds); e, t = _edge_rule_variant(d, ds, variant)
        return not (np.array_equal(e, r["edge"][3:-3, 3:-3] > 0) and np.array_equal(t, r["total_area"][3:-3, 3:-3] > 0))
    assert not differs("ties_400", None) and not differs("ramp_5208", None)                     # the variant code itself is the rule
    assert differs("ties_400", "400_ge") and differs("ties_3pct", "pct_ge") and differs("half_even", "half_ge")
    assert differs("ramp_5000.33", "fp64")                                                       # the FP32 quotient of 30002 rounds up to 6.0f: invalid; in FP64 it is below 6
    assert differs("ramp_1006", "reciprocal") and differs("ramp_3400", "reciprocal")          # a product with the reciprocal is not the division: 6 m itself would be valid
    p = R.depth_norm_products(fr["norm_510"][0])
    assert not np.array_equal(np.clip(np.floor(p + np.float32(0.5)), 0, 255).astype(np.uint8), R.depth_norm(fr["norm_510"][0]))      # round half up
    for names, _ in S.front_batches(w, h):                                                        # a maximum taken from a neighbour's slot changes the normalised depth
        ds_ = [fr[n][0] for n in names]
        for a in range(3):
            b = (a + 1) % 3
            if ds_[a].max() > 0 and ds_[b].max() > 0:
                wrong = np.clip(np.rint(ds_[a].astype(np.float32) * np.float32((1.0 / float(ds_[b].max())) * 255)), 0, 255).astype(np.uint8)
                assert not np.array_equal(wrong, R.depth_norm(ds_[a])), (names, a)
