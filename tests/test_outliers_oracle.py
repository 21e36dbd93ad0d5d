"""CPU tests of tests/outliers_oracle.py, the numpy yardstick of the outlier filters: against naive double loops on small clouds, on
clouds with planted strays, and that no input of the GPU mask tests lies in the threshold band."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import outliers_oracle as O  # noqa: E402


def small_clouds():
    r = np.random.RandomState(3)
    dup = r.random_sample((40, 3)).astype(np.float32)
    dup[5:25] = dup[2]                                          # 21 coincident points: more than k + 1 at k = 7
    return [O.sphere(40, 4), O.lattice(3), dup, r.random_sample((1, 3)).astype(np.float32), r.random_sample((2, 3)).astype(np.float32),
            (O.far_ellipsoid(33, 2))]


@pytest.mark.parametrize("k", [1, 7, 16, 31])
def test_mean_dist_equals_the_naive_loop(k):
    for p in small_clouds():
        got, want = O.mean_dist(p, k), O.naive_mean_dist(p, k)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (len(p), k)


def test_mean_dist_closed_forms():
    assert np.array_equal(O.mean_dist(np.float32([[1, 2, 3]]), 16), np.float32([0]))                    # n = 1
    assert np.array_equal(O.mean_dist(np.float32([[0, 0, 0], [3, 4, 0]]), 16), np.float32([5, 5]))       # n = 2: the one other point
    assert not O.mean_dist(np.tile(np.float32([[3, -1, 2]]), (100, 1)), 16).any()                       # all coincident
    line = np.arange(5, dtype=np.float32)[:, None] * np.float32([[1, 0, 0]])
    assert np.array_equal(O.mean_dist(line, 2), np.float32([1.5, 1, 1, 1, 1.5]))


@pytest.mark.parametrize("cap", [None, 1, 4])
def test_radius_count_equals_the_naive_loop(cap):
    for p in small_clouds():
        for radius in (0.25, 1.0, 1.5):
            assert np.array_equal(O.radius_count(p, radius, cap), O.naive_radius_count(p, radius, cap))


def test_radius_boundary_is_inclusive_on_the_lattice():
    cnt = O.radius_count(O.lattice(9), 1.0)
    assert cnt.min() == 3 and cnt.max() == 6                    # d2 = r2 = 1 exactly: the axis neighbours count
    assert O.radius_count(O.lattice(9), np.nextafter(np.float32(1.0), np.float32(0.0))).max() == 0


def test_threshold_is_float64_mean_and_sample_std():
    md = np.float32([1, 2, 3, 4])
    mu, sigma, thr = O.threshold(md, 2.0)
    assert mu == 2.5 and sigma == np.sqrt(5.0 / 3.0) and thr == 2.5 + 2.0 * np.sqrt(5.0 / 3.0)
    assert O.threshold(np.float32([7]), 1.0) == (7.0, 0.0, 7.0)
    keep, st, _ = O.statistical_keep(np.tile(np.float32([[3, -1, 2]]), (50, 1)), 16, 2.0)
    assert st == (0.0, 0.0, 0.0) and np.array_equal(keep, np.arange(50))        # all duplicates: everything stays


@functools.lru_cache(maxsize=None)
def mask_sorted_d2(name):
    return O.sorted_d2(O.mask_cloud(name), 32)


def mask_mean_dist(name, k):
    sd2 = mask_sorted_d2(name)
    return O.mean_dist_from_sorted(sd2, len(sd2), k)


@pytest.mark.parametrize("k", O.MASK_K)
@pytest.mark.parametrize("name,n,seed,ratios", [("planted2000", 2000, 1, (1.0,)), ("planted4097", 4097, 2, (1.0, 2.0))])
def test_planted_strays_are_what_is_removed(name, n, seed, ratios, k):
    p, ns = O.planted(n, seed)
    assert ns == {1: 36, 2: 30}[seed] and len(p) == n + ns
    for ratio in ratios:
        keep, _, _ = O.statistical_keep(p, k, ratio, md=mask_mean_dist(name, k))
        assert np.array_equal(keep, np.arange(n)), (k, ratio)  # all strays, nothing else


@pytest.mark.parametrize("k", O.MASK_K)
@pytest.mark.parametrize("name", O.MASK_CLOUDS)
def test_threshold_band_is_empty_on_the_gpu_inputs(name, k):
    md = mask_mean_dist(name, k)
    for ratio in O.MASK_RATIO:
        thr = O.threshold(md, ratio)[2]
        assert O.band(md, thr) > O.BAND, (name, k, ratio, O.band(md, thr))
