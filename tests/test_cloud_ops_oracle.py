"""tests/cloud_ops_oracle.py held to oracle/upsample.py and to itself, and the tie inputs of tests/test_cloud_ops_gpu.py held to what
they are for.  CPU only.

  * the float32 replay of the normalisation equals oracle.upsample.normalize_point_cloud in float32 bit for bit -- centroid, furthest
    and every coordinate, NaNs in the same places -- at every size the GPU test uses, and lies within normalize_f64's bound of the
    float64 result;
  * the k-NN oracle equals oracle.upsample.extract_knn_patch_idx;
  * every tie cloud that is to exercise the radix select's collect pass has, by the oracle's distances alone, a k-th distance shared
    by more points than the quota takes, spread over more than one 256-point chunk and more than one wave of a chunk, and a point that
    only a count carried across waves and chunks keeps out;
  * np.nanmean / np.nanstd agree with exact sums (math.fsum) within nan_mean_std's bounds."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ops_oracle as CO  # noqa: E402
from cloud_ops_oracle import F32  # noqa: E402

from oracle import upsample as OU  # noqa: E402

NORM_N = [1, 2, 63, 64, 65, 256, 300, 8192, 24576]               # the sizes of tests/test_cloud_ops_gpu.py


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    nan = np.isnan(b)
    return a.shape == b.shape and bool(np.isnan(a)[nan].all()) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("n", NORM_N)
def test_replay_equals_normalize_point_cloud(n):
    for b, first in ((3, 0), (1, 1), (70, 2) if n in (65, 24576) else (2, 2)):
        p = CO.offcentre_clouds(b, n, seed=n + b, first=first)
        out, c, f = CO.normalize_replay(p)
        with np.errstate(invalid="ignore", divide="ignore"):
            w_out, w_c, w_f = OU.normalize_point_cloud(p)                        # [B, N, 3]: axis 1
            one = OU.normalize_point_cloud(p[0])                                 # [N, 3]: axis 0
        assert w_out.dtype == F32 and w_c.dtype == F32 and w_f.dtype == F32
        assert same_bits_or_nan(c, w_c[:, 0, :]) and same_bits_or_nan(f, w_f[:, 0, 0]) and same_bits_or_nan(out, w_out)
        assert same_bits_or_nan(out[0], one[0]) and same_bits_or_nan(c[0], one[1][0]) and same_bits_or_nan(f[0], one[2][0, 0])
        assert np.isnan(out).all() == (n == 1) and (n == 1 or np.isfinite(out).all())
        ref = CO.normalize_f64(p)
        assert (np.abs(c - ref["centroid"]) <= ref["centroid_bound"]).all()
        assert (np.abs(f - ref["furthest"]) <= ref["furthest_bound"]).all()
        if n > 1:
            assert (np.abs(out - ref["out"]) <= ref["out_bound"]).all()
            assert np.abs(np.linalg.norm(ref["out"], axis=2).max(1) - 1.0).max() < 1e-12    # the furthest point lands on the unit sphere


def test_replay_on_coincident_points():
    """n copies of a point whose sums are exact: centroid = the point, furthest = 0, every coordinate NaN, in both."""
    for n in (2, 300, 24576):
        p = np.empty((2, n, 3), F32)
        p[0], p[1] = (0.5, -2.0, 1.25), (3.0, 0.25, -0.75)
        out, c, f = CO.normalize_replay(p)
        with np.errstate(invalid="ignore", divide="ignore"):
            w_out, w_c, w_f = OU.normalize_point_cloud(p)
        assert np.array_equal(c, p[:, 0]) and (f == 0).all() and np.isnan(out).all()
        assert np.array_equal(w_c[:, 0], c) and (w_f == 0).all() and np.isnan(w_out).all()


def test_denormalize_is_two_roundings():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((4, 50, 3)).astype(F32)
    c = (rng.standard_normal((4, 3)) * 100).astype(F32)
    f = np.array([1e-3, 1.0, 37.5, 1e4], F32)
    got = CO.denormalize(x, c, f)
    prod = (x.astype(np.float64) * f.astype(np.float64)[:, None, None]).astype(F32)           # exact product, rounded once
    want = (c.astype(np.float64)[:, None, :] + prod.astype(np.float64)).astype(F32)           # exact sum, rounded once
    assert np.array_equal(got, want)
    fused = (c.astype(np.float64)[:, None, :] + x.astype(np.float64) * f.astype(np.float64)[:, None, None]).astype(F32)
    assert (fused != want).any()                                                              # a contracted build would show
    # oracle.upsample.upsample_cloud's own lines: pred = pc_c + fine * pc_f, merged = pred * f0 + c0
    assert np.array_equal(got, c[:, None, :] + x * f[:, None, None])


KNN_SHAPES = [(1, 1, 1), (3, 2, 2), (5, 5, 5), (257, 4, 256), (1000, 5, 1000), (9261, 3, 1024)]


@pytest.mark.parametrize("shape", KNN_SHAPES, ids=["-".join(map(str, s)) for s in KNN_SHAPES])
def test_knn_equals_extract_knn_patch_idx(shape):
    n, m, k = shape
    pc, q = CO.random_case(2, n, m, seed=n)
    pc[1, n // 2] = pc[1, 0]                                                     # a duplicate: the tie goes to the lower index
    for c in range(2):
        idx, srt = CO.knn(q[c], pc[c], k)
        assert idx.dtype == np.int32 and np.array_equal(idx, OU.extract_knn_patch_idx(q[c], pc[c], k))
        assert (np.diff(srt, axis=1) >= 0).all()
        d2 = CO.sqdist(q[c], pc[c])
        for j in range(m):                                                        # ascending (distance, index), nothing nearer left out
            key = list(zip(d2[j][idx[j]].tolist(), idx[j].tolist()))
            assert key == sorted(key) and len(set(idx[j].tolist())) == k
            assert k == n or d2[j][np.setdiff1d(np.arange(n), idx[j])].min() >= d2[j][idx[j][-1]]
    assert np.array_equal(CO.knn_batch(q, pc, k)[1], CO.knn(q[1], pc[1], k)[0])


@pytest.mark.parametrize("case", CO.TIE_CASES, ids=[c[0] for c in CO.TIE_CASES])
def test_tie_inputs_hold_the_ties_they_are_for(case):
    name, build, arg, ks, must = case
    pc, q = build(arg)
    assert pc.dtype == F32 and q.dtype == F32 and pc.shape[0] == q.shape[0] >= 2
    assert pc.shape[1] == (arg ** 3 if name.startswith("lattice") else arg)
    assert not np.array_equal(pc[0], pc[1])
    for k in ks:
        assert k <= pc.shape[1]
        for (c, j) in must:
            t = CO.tie_facts(q[c, j], pc[c], k)
            print("%s k %d cloud %d query %d: %s" % (name, k, c, j, t))
            if name.startswith("copies") and k > CO.COPIES:
                continue                                                          # past the copies: the k-th distance is an ordinary one
            assert t["cut"], "%s k %d (%d, %d): all %d points at the k-th distance are taken" % (name, k, c, j, t["shared"])
            assert t["chunks"] > 1 and t["waves"] > 1 and t["carry_matters"] and t["chunk_carry_matters"]
    if name.startswith("copies"):
        for c in range(2):                                                        # the copies are the tie for every k up to 600
            d2 = CO.sqdist(q[c, :1], pc[c])[0]
            dP = CO.sqdist(q[c, :1], q[c, 1:2])[0, 0]
            assert (d2 == dP).sum() == CO.COPIES and (d2 < dP).sum() < 50
            assert len(set((np.nonzero(d2 == dP)[0] // CO.CHUNK).tolist())) >= (pc.shape[1] - 300) // CO.CHUNK
    if name.startswith("lattice"):
        d2 = CO.sqdist(q[0, 3:4], pc[0])[0]
        assert (d2 == d2.min()).sum() == 8                                        # the cell-centre query: eight nearest at once
    if name.startswith("identical"):
        assert np.signbit(q[2, 0]).all() and not np.signbit(pc[2]).any()
        d = q[2, 0] - pc[2, 0]
        assert np.signbit(d).all() and not np.signbit(CO.sqdist(q[2, :1], pc[2])).any()      # -0 differences, +0 distance


def test_nan_mean_std_against_exact_sums():
    for (b, n) in ((1, 1), (1, 255), (3, 257), (2, 100000)):
        for turn in range(4):
            x, kinds = CO.stat_rows(b, n, turn, seed=n)
            r = CO.nan_mean_std(x)
            for i, kind in enumerate(kinds):
                v = [float(t) for t in x[i] if not math.isnan(t)]
                if kind == "allnan":
                    assert not v and math.isnan(r["mean"][i]) and math.isnan(r["std"][i])
                    continue
                mean = math.fsum(v) / len(v)
                std = math.sqrt(math.fsum((t - mean) ** 2 for t in v) / len(v))
                assert abs(r["mean"][i] - mean) <= r["mean_bound"][i] and abs(r["std"][i] - std) <= r["std_bound"][i]
                if kind == "constant":
                    assert r["std"][i] == 0.0 and r["std_bound"][i] == 0.0 and r["mean"][i] == float(x[i, 0])
                if kind == "scattered" and n > 1:
                    assert 0 < len(v) < n
    assert set(k for t in range(4) for k in CO.stat_rows(1, 1, t, 0)[1]) == set(CO.ROW_KINDS)
