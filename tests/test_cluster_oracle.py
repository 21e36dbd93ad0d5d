"""tests/cluster_oracle.py held to its naive twin, to hand-worked cases and, where scikit-learn is installed, to DBSCAN(algorithm="brute");
and the refusals of dis-pu_amd/clusters.py that need no device."""
import numpy as np
import pytest

import cluster_oracle as O

G = 1.0 / 16.0                                                   # coordinates on a 2^-4 grid: every d2 below is exact in fp32


def same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("eps,min_points", [(0.3, 1), (0.3, 3), (0.45, 4), (0.2, 2), (5.0, 41)])
def test_oracle_equals_naive_twin(seed, eps, min_points):
    g = np.random.RandomState(seed)
    n = int(g.randint(1, 41))
    p = (g.randint(0, 24, (n, 3)) * G).astype(np.float32)       # a coarse grid: many exact ties and duplicates
    if seed % 2:
        p = g.rand(n, 3).astype(np.float32)
    same(O.dbscan(p, eps, min_points), O.naive(p, eps, min_points))


def test_hand_chain_and_noise():
    # 0 - 1 - 2 at spacing 1, a far point 3: eps 1 includes the boundary
    p = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [9, 0, 0]])
    labels, core, sizes = O.dbscan(p, 1.0, 2)
    assert labels.tolist() == [0, 0, 0, -1] and core.tolist() == [True, True, True, False] and sizes.tolist() == [3]
    labels, core, sizes = O.dbscan(p, 1.0, 3)                    # only the middle point has three within eps: the ends are borders
    assert labels.tolist() == [0, 0, 0, -1] and core.tolist() == [False, True, False, False] and sizes.tolist() == [3]
    labels, core, sizes = O.dbscan(p, 1.0, 1)                    # Euclidean cluster extraction: everything is core
    assert labels.tolist() == [0, 0, 0, 1] and core.all() and sizes.tolist() == [3, 1]
    labels, core, sizes = O.dbscan(p, np.nextafter(np.float32(1.0), np.float32(0.0)), 2)
    assert labels.tolist() == [-1] * 4 and not core.any() and sizes.shape == (0,)


def test_hand_numbering_follows_first_core_index():
    p = np.float32([[9, 0, 0], [0, 0, 0], [9, G, 0], [0, G, 0]])
    labels, _, sizes = O.dbscan(p, 2 * G, 2)
    assert labels.tolist() == [0, 1, 0, 1] and sizes.tolist() == [2, 2]
    labels, _, _ = O.dbscan(p[[1, 0, 3, 2]], 2 * G, 2)
    assert labels.tolist() == [0, 1, 0, 1]                        # the numbering follows the permuted first index


def bridge(first):
    """two blobs of 4 coincident-ish points at x = 0 and x = 8 G, and one bridge point at x = 4 G within eps = 4 G of one core point of
    each, equidistant; first: which blob comes first in the input"""
    a = np.float32([[0, 0, 0], [0, G, 0], [0, 0, G], [0, G, G]])
    b = a + np.float32([8 * G, 0, 0])
    blobs = [a, b] if first == "a" else [b, a]
    return np.concatenate(blobs + [np.float32([[4 * G, 0, 0]])])


@pytest.mark.parametrize("first", ["a", "b"])
def test_hand_bridge_point_never_joins_two_clusters(first):
    p = bridge(first)
    labels, core, sizes = O.dbscan(p, 4 * G, 4)                   # the bridge sees itself + (0,0,0) + (8G,0,0) = 3 < 4: not core
    assert core.tolist() == [True] * 8 + [False]
    assert labels[:8].tolist() == [0] * 4 + [1] * 4
    assert labels[8] == 0 and sizes.tolist() == [5, 4]            # equidistant: the core point of smaller index, row 0 of the first blob
    same(O.dbscan(p, 4 * G, 4), O.naive(p, 4 * G, 4))


def test_hand_coincident_points():
    p = np.zeros((7, 3), np.float32) + np.float32(0.5)
    assert O.dbscan(p, 0.1, 7)[0].tolist() == [0] * 7
    assert O.dbscan(p, 0.1, 8)[0].tolist() == [-1] * 7


def test_keep_order():
    labels = np.int32([0, 0, 1, 1, 2, -1, 3, 3, 3])
    sizes = np.int32([2, 2, 1, 3])
    assert O.keep(labels, sizes, 1, 1).tolist() == [6, 7, 8]
    assert O.keep(labels, sizes, 2, 1).tolist() == [0, 1, 6, 7, 8]          # the size tie goes to id 0
    assert O.keep(labels, sizes, 32, 2).tolist() == [0, 1, 2, 3, 6, 7, 8]
    assert O.keep(labels, sizes, 3, 4).tolist() == []


@pytest.mark.parametrize("n,eps,min_points", O.SHELL_CASES)
def test_against_scikit_learn(n, eps, min_points):
    sk = pytest.importorskip("sklearn.cluster")
    p = O.shells(n)
    labels, core, _ = O.dbscan(p, eps, min_points)
    m = sk.DBSCAN(eps=float(np.float32(eps)), min_samples=min_points, algorithm="brute").fit(p.astype(np.float64))
    sk_core = np.zeros(n, bool)
    sk_core[m.core_sample_indices_] = True
    assert np.array_equal(core, sk_core)
    assert np.array_equal(labels[core], m.labels_[core])
    assert np.array_equal(labels == -1, m.labels_ == -1)


def test_refusals_need_no_device():
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import clusters as M
    for fn in (M.dbscan, M.keep_clusters):
        with pytest.raises(ValueError, match="ROCm device"):
            fn(torch.zeros(8, 3), 0.1)
        with pytest.raises(ValueError, match="ROCm device or a list"):
            fn(np.zeros((8, 3), np.float32), 0.1)
        with pytest.raises(ValueError, match="at least one cloud"):
            fn([], 0.1)
