"""CPU tests of tests/attributes_oracle.py, the numpy yardstick of the cross-cloud k-NN and the attribute transfer: at k = 3 against the
project's CPU oracle of three_nn (and the reference's own function where it was built), and by hand on cases whose answer is known."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import attributes_oracle as A  # noqa: E402

SEED = 0                                                        # chosen so that the gap condition below holds


def test_k3_equals_three_nn():
    """random clouds, n = 300 queries against m = 200 references.  First a condition on the input: the four smallest d2 of every query
    differ pairwise by a relative gap above 1e-5, so neither a tie rule nor a contracted multiply-add can change the answer."""
    from oracle import oracle as O
    from oracle import ref as R
    r = np.random.RandomState(SEED)
    q = r.random_sample((300, 3)).astype(np.float32)
    p = r.random_sample((200, 3)).astype(np.float32)
    _, d4 = A.knn_cross(q, p, 4)
    d4 = d4.astype(np.float64)
    gaps = (d4[:, 1:] - d4[:, :-1]) / d4[:, 1:]                 # ascending: neighbouring gaps bound every pairwise gap from below
    assert gaps.min() > 1e-5, gaps.min()
    idx, d2 = A.knn_cross(q, p, 3)
    dist, ti = O.three_nn(q[None], p[None])
    assert np.array_equal(idx, ti[0]) and np.array_equal(d2.view(np.uint32), dist[0].view(np.uint32))
    if R.available():
        dist, ti = R.threenn(q[None], p[None])
        assert np.array_equal(idx, ti[0]) and np.array_equal(d2.view(np.uint32), dist[0].view(np.uint32))


def test_keys_against_a_naive_double_loop():
    """ties by index, duplicates and d2 = 0 on a small integer lattice"""
    r = np.random.RandomState(1)
    p = r.randint(0, 3, (40, 3)).astype(np.float32)
    q = r.randint(0, 3, (17, 3)).astype(np.float32)
    for k in (1, 3, 8):
        idx, d2 = A.knn_cross(q, p, k)
        for i in range(len(q)):
            d = [np.float32(np.float32(np.float32((q[i, 0] - p[j, 0]) ** 2) + np.float32((q[i, 1] - p[j, 1]) ** 2))
                            + np.float32((q[i, 2] - p[j, 2]) ** 2)) for j in range(len(p))]
            order = sorted(range(len(p)), key=lambda j: (d[j], j))[:k]
            assert list(idx[i]) == order and list(d2[i]) == [d[j] for j in order]


def test_query_on_a_reference_point_takes_its_attribute():
    r = np.random.RandomState(2)
    p = r.random_sample((50, 3)).astype(np.float32)
    feat = (r.random_sample((50, 2)) + 0.5).astype(np.float32)
    labels = r.randint(0, 9, 50).astype(np.int32)
    q = p[[7, 31, 0]]
    near = A.transfer(q, p, feat, k=3, mode="nearest")
    assert np.array_equal(near, feat[[7, 31, 0]])
    idw = A.transfer(q, p, feat, k=3, mode="idw")
    assert np.all(np.abs(idw - feat[[7, 31, 0]]) <= 1e-6 * np.abs(feat[[7, 31, 0]]))
    assert np.array_equal(A.nearest_label(q, p, labels), labels[[7, 31, 0]])


def test_two_equidistant_references_give_the_mean():
    p = np.float32([[-1, 0, 0], [1, 0, 0], [0, 50, 0]])
    feat = np.float32([[2.0, -4.0], [6.0, 8.0], [1000.0, 1000.0]])
    q = np.float32([[0, 0, 0], [0, 0, 3]])
    out = A.transfer(q, p, feat, k=2, mode="idw")
    assert np.array_equal(out, np.float32([[4.0, 2.0], [4.0, 2.0]]))
    idx, _ = A.knn_cross(q, p, 2)
    assert np.array_equal(idx, np.int32([[0, 1], [0, 1]]))      # equal d2: the smaller index first
    assert np.array_equal(A.nearest_label(q, p, np.int32([5, 6, 7])), np.int32([5, 5]))


def test_fewer_references_than_k_pads_and_interpolates_over_them():
    p = np.float32([[0, 0, 0], [3, 0, 0]])
    feat = np.float32([[1.0], [5.0]])
    q = np.float32([[1, 0, 0]])
    idx, d2 = A.knn_cross(q, p, 4)
    assert np.array_equal(idx, np.int32([[0, 1, -1, -1]]))
    assert np.array_equal(d2, np.float32([[1.0, 4.0, np.inf, np.inf]]))
    out = A.transfer(q, p, feat, k=4, mode="idw")                # weights 1 and 1/4: (1 + 5/4) / (5/4) = 1.8
    assert out.shape == (1, 1) and out[0, 0] == np.float32((1.0 + 0.25 * 5.0) / 1.25)
    assert np.array_equal(A.transfer(q, p, feat, k=4, mode="nearest"), np.float32([[1.0]]))
