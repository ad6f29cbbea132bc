"""CPU: the host twin sindh_cloud_filter_outliers (csrc/host/cloud_filter.cpp: the arithmetic of csrc/host/cloud_filter.hpp over a grid search of its own) against the
literal numpy restatement of the contract in tests/cloud_filter_ref.py: the bits of the distances, the bytes of the three stats doubles, the kept indices.  The contract
is restated from PCL 1.10 (StatisticalOutlierRemoval over KdTreeFLANN); parity with a real PCL build is unpinned, and nothing here claims it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import cloud_filter_ref as R
import cloud_filter_scene as S
from sindslam_amd.cloud import MAX_MEAN_K, POINT_DTYPE, STATS_DTYPE, filterOutliersHost

SIND_E_ARG, SIND_E_CAPACITY = -1, -5


@pytest.mark.parametrize("name,mean_k", S.CASES)
def test_twin_equals_the_literal_contract(name, mean_k):
    p = S.SCENE[name](mean_k); ref = S.reference(name, mean_k); got = S.twin(name, mean_k)
    S.assert_equals_reference(got, p, ref)
    assert got["n_ring"] == 0 and got["n_brute"] == 0


def test_the_scenes_are_what_they_claim():
    """the properties the scenes exist for, on the literal reference"""
    r = S.reference("random_far", 100); p = S.random_far()
    assert r["valid"] == int(np.isfinite(np.stack([p["x"], p["y"], p["z"]], 1)).all(1).sum()) < len(p) and r["degenerate"] == 0
    kept = np.zeros(len(p), bool); kept[r["keep"]] = True
    fin = np.isfinite(p["x"]) & np.isfinite(p["y"]) & np.isfinite(p["z"])
    assert kept[~fin].all()                                             # non-finite points are never removed
    far = np.arange(4000, 4061); far = far[fin[far]]
    assert (r["distances"][far] > 500).all() and not kept[far].any()   # the far cluster's and the lone point's neighbours come from the main cloud
    assert (r["distances"][~fin] == 0).all()
    r = S.reference("lattice", 100)
    assert len(np.unique(r["distances"])) == 18 and len(r["keep"]) == 1528      # mass ties at the k-th distance
    for k in S.MEAN_KS:
        r = S.reference("coincident", k)
        assert (r["distances"] == 0).all() and r["threshold"] == 0.0 and len(r["keep"]) == 150
        r = S.reference("exactly_k_plus_one", k); assert r["degenerate"] == 0 and r["valid"] == k + 1
        r = S.reference("k_finite_among_nans", k); assert r["degenerate"] == 1 and r["valid"] == k and len(r["keep"]) == 2 * k + 7 and r["threshold"] == 0.0
    assert S.reference("planar", 50)["keep"].tolist().count(7) == 0     # the in-plane outlier goes
    x = S.offset()["x"].astype(np.float64) * 1024; assert (x == np.round(x)).all()      # coordinates on the 2^-10 lattice of FP32 at 1e4
    r = S.reference("two_points", 1); assert np.isnan(r["threshold"]) and np.isnan(r["stddev"]) and len(r["keep"]) == 2 and r["distances"][0] == r["distances"][1] > 0
    assert S.f64_bytes(r["threshold"]) == bytes.fromhex("000000000000f87f")
    assert S.reference("n0", 1)["degenerate"] == 1 and S.reference("n64", 1)["degenerate"] == 0 and S.reference("n65", 50)["degenerate"] == 0


@pytest.mark.parametrize("mul", [0.0, -0.5, 2.5])
def test_other_multipliers(mul):
    p = S.planar(); got, = filterOutliersHost([p], 30, mul)
    S.assert_equals_reference(got, p, R.filter_outliers(p, 30, mul))


def test_batch_of_three_with_an_empty_and_a_degenerate_cloud():
    clouds = [S.offset()[:700], S.tiny(0)(), S.k_finite_among_nans(50)]
    got = filterOutliersHost(clouds, 50, 1.0)
    for g, p in zip(got, clouds):
        S.assert_equals_reference(g, p, R.filter_outliers(p, 50, 1.0))
    assert [g["degenerate"] for g in got] == [0, 1, 1] and len(got[1]["points"]) == 0


def test_mean_distances_against_a_kd_tree():
    """scipy's cKDTree as an independent search: FP64 distances against the contract's FP32 ones, equal to a relative 1e-5"""
    from scipy.spatial import cKDTree
    p = S.random_far(); got = S.twin("random_far", 100)
    xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64); fin = np.isfinite(xyz).all(1)
    d, _ = cKDTree(xyz[fin]).query(xyz[fin], k=101)
    assert np.allclose(got["distances"][fin], d[:, 1:].mean(1), rtol=1e-5, atol=0)


def test_errors_and_capacity():
    from sindslam_amd.cloud import _host_lib
    L = _host_lib(); p = S.planar(); n = np.array([len(p)], np.int32); out = np.zeros(len(p), POINT_DTYPE); n_out = np.full(1, 77, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda k, mul, cap: L.sindh_cloud_filter_outliers(1, ptr(p), len(p), ptr(n), k, C.c_double(mul), ptr(out), cap, ptr(n_out), None, None)
    for k, mul in ((0, 1.0), (MAX_MEAN_K + 1, 1.0), (50, float("nan")), (50, float("inf"))):
        assert call(k, mul, len(p)) == SIND_E_ARG and n_out[0] == 77
    assert call(MAX_MEAN_K, 1.0, len(p)) == 0 and 0 < n_out[0] < len(p)
    kept = int(n_out[0])
    assert call(MAX_MEAN_K, 1.0, kept - 1) == SIND_E_CAPACITY and n_out[0] == kept
    assert call(MAX_MEAN_K, 1.0, kept) == 0
    assert STATS_DTYPE.itemsize == 40


def test_a_sanitizer_build_of_the_host_twin_runs_clean_as_its_own_process(tmp_path):
    """a C++ main over sindh_cloud_filter_outliers and csrc/host/cloud_filter.cpp with -fsanitize=address,undefined, run as a program of its own: every array exactly
    as long as the call may touch.  Nothing is loaded into python."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cloudfilter_sanitize")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "sindslam_amd", "csrc"), "sanitize-cloudfilter", "OUT=" + exe], check=True, capture_output=True, text=True)
    records = []                                                       # (clouds, mean_k, mul, out_cap or None, expected rc)
    for name in ("random_far", "lattice", "coincident", "planar", "collinear", "offset", "n0", "n1", "n65"):
        records.append(([S.SCENE[name](100)], 100, 1.0, None, 0))
    records.append(([S.exactly_k_plus_one(MAX_MEAN_K), S.tiny(0)(), S.k_finite_among_nans(MAX_MEAN_K)], MAX_MEAN_K, 0.5, None, 0))
    records.append(([S.planar()], 50, 1.0, 100, SIND_E_CAPACITY))
    records.append(([S.planar()], MAX_MEAN_K + 1, 1.0, None, SIND_E_ARG))
    blob = struct.pack("<i", len(records)); want = []
    for clouds, k, mul, cap, rc in records:
        B = len(clouds); stride = max(len(c) for c in clouds); cap = stride if cap is None else cap
        pts = np.zeros((B, stride), POINT_DTYPE); n = np.array([len(c) for c in clouds], np.int32)
        for b, c in enumerate(clouds):
            pts[b, :len(c)] = c
        blob += struct.pack("<5id", B, stride, k, cap, rc, mul) + n.tobytes() + pts.tobytes()
        line = str(rc)
        if rc != SIND_E_ARG:
            for c, g in zip(clouds, filterOutliersHost(clouds, k, mul)):
                i = np.arange(1, len(c) + 1, dtype=np.uint32); x = int(np.bitwise_xor.reduce(g["distances"].view(np.uint32) * i)) if len(c) else 0
                q = g["points"][:cap]; j = np.arange(1, len(q) + 1, dtype=np.int64)
                s = int(((q["b"].astype(np.int64) + 2 * q["g"].astype(np.int64) + 3 * q["r"].astype(np.int64)) * j).sum())
                line += f" {len(g['points'])} {g['valid']} {g['degenerate']} {x} {s}"
        want.append(line)
    path = tmp_path / "records.bin"; path.write_bytes(blob)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.splitlines() == want
