"""CPU: the numpy restatement of the large-motion test (motion_ref.decide) equals the oracle's endFlow / endFlow2 / largeMotion on real frames, flagged and not,
and on its own it separates both members of every pair of on-the-rule cases that test_large_motion_gpu.py runs -- so a GPU result equal to it is on the rule."""
import numpy as np
import pytest

import motion_ref as R
import motion_scene as M
import oracle_lib as O


@pytest.mark.parametrize("w,h,what,frames", [(192, 144, (6, 2), (2, 3)), (192, 144, (0, 0), (2,)), (192, 144, (8, 0), (6,)), (128, 72, (3, 1), (2,)),
                                             (320, 240, ("walkers", 0), (2, 3))])
def test_restatement_equals_the_oracle_on_real_frames(w, h, what, frames):
    bgr, _ = M.stream(w, h, what); K = M.intrinsics(w); seen = set()
    fw, fh = int(np.float32(0.6) * w), int(np.float32(0.6) * h)
    for f in frames:
        det = O.DynaDetect(bgr[f - 1], bgr[f - 2], *K); det.flow_only(bgr[f]); e1, e2, lm = det.motion()
        # the flow the decision is taken on: flow(n, n - 2) on the 0.6 grid, negated (DD:1075-1080)
        g = [O.resize_u8(O.bgr2gray(bgr[k]), fw, fh) for k in (f, f - 2)]
        flow = -O.deepflow(g[0], g[1])
        r = R.decide(flow[..., 0], flow[..., 1], w, h)
        assert (r["endFlow"], r["endFlow2"], r["flag"]) == (e1, e2, int(lm)), (w, h, what, f)
        assert r["hist"].sum() == fw * fh
        if (w, h, what) in M.FLAGS:
            assert int(lm) == M.FLAGS[(w, h, what)][f - 2], (w, h, what, f)
        seen.add(int(lm))
    assert len(frames) == 1 or seen == {0, 1}                       # the two-frame cases hold a flagged and an unflagged frame


def test_the_threshold_counts_the_full_frame():
    """totalpixel is 0.36 W H in FP32, not fw * fh: they differ whenever 0.6 W is not an integer (64 x 72: 1634 pixels on the grid, 1658.88 in the rule)"""
    for fw, fh, W, H in R.SIZES:
        assert (fw, fh) == (int(np.float32(0.6) * W), int(np.float32(0.6) * H))
    assert 38 * 43 == 1634 and abs(float(R.threshold(64, 72)) - 0.3 * 1658.88) < 1e-3 and int(R.threshold(64, 72)) != int(0.3 * 1634)
    assert float(R.threshold(640, 480)) == pytest.approx(0.3 * 110592, rel=1e-6)


@pytest.mark.parametrize("fw,fh,W,H", R.SIZES)
def test_cases_are_on_the_rule(fw, fh, W, H):
    cs = R.cases(fw, fh, W, H); res = {n: R.decide(c["u"], c["v"], W, H) for n, c in cs.items()}
    K = int(np.floor(R.threshold(W, H)))
    for n, c in cs.items():
        r = res[n]
        assert r["hist"].sum() == fw * fh, n
        if c["expect"] is not None:
            assert (r["flag"], r["endFlow"], r["endFlow2"]) == c["expect"], (n, r["flag"], r["endFlow"], r["endFlow2"])
    for flagged, calm in R.PAIRS:
        assert res[flagged]["flag"] == 1 and res[calm]["flag"] == 0, (flagged, calm)
    # the cumulative count at bin endFlow: floor(0.3f * totalpixel) exactly, and that plus one
    a, b = res["count/at_floor"], res["count/floor_plus_one"]
    assert int(a["hist"][:a["endFlow"] + 1].sum()) == K and int(b["hist"][:b["endFlow"] + 1].sum()) == K + 1
    assert a["endFlow2"] == a["endFlow"] + 1 and b["endFlow2"] == b["endFlow"]
    # 1530 / max just above / at / just below an integer: same histogram bins, endFlow 15 / 15 / 14
    assert [res["integer/" + t]["endFlow"] for t in ("above", "exact", "below")] == [15, 15, 14]
    assert len({float(res["integer/" + t]["max"]) for t in ("above", "exact", "below")}) == 3
    # round half to even: the tie pixels sit in the even bin
    assert res["half/even"]["hist"][12] == K + 1 and res["half/odd"]["hist"][24] == K + 1 and res["half/odd_up"]["hist"][8] == K + 1
    for n, m in (("half/even", 127.5), ("half/odd", 63.75), ("half/odd_up", 255.0)):
        assert float(np.float32(255.0 / m)) == 255.0 / m                          # a is exact, so is the product: a true tie
    # the maximum at the first / last index only
    for n, idx in (("ends/first", 0), ("ends/last", fw * fh - 1)):
        mag = np.hypot(cs[n]["u"].astype(np.float64), cs[n]["v"].astype(np.float64)).ravel()
        assert int(np.argmax(mag)) == idx and (mag == mag.max()).sum() == 1, n
    # ranges: 1530 / 1e-20 does not fit an int; m * m is subnormal there
    t = res["range/tiny"]; assert t["endFlow"] == R.INT_MIN and t["flag"] == 1 and 0 < float(t["max"]) < 2e-20 and t["hist"][3] >= K + 1
    assert float(np.float32(1e-20) * np.float32(1e-20)) < float(np.finfo(np.float32).tiny)
    assert res["zero"]["hist"][0] == fw * fh and float(res["zero"]["max"]) == 0.0 and res["zero"]["flag"] == 1
    assert {res["general/calm"]["flag"], res["general/fast"]["flag"]} == {0, 1}
    # batches: every case runs; distinct maxima; the largest neither first nor last; an all-zero image in every batch of 3 and 5
    names = list(cs)
    for B in (1, 3, 5):
        bs = R.batches(names, B)
        assert {n for b in bs for n in b} == set(names) and all(len(b) == B for b in bs)
        if B > 1:
            for b in bs:
                mx = [float(res[n]["max"]) for n in b]
                assert len(set(mx)) == B and 0 < int(np.argmax(mx)) < B - 1 and "zero" in b, b
                assert {res[n]["flag"] for n in b} == {0, 1}, b
