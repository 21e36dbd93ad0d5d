"""CPU tests of tests/normals_oracle.py, the numpy yardstick of dispu_pca_normals_segments, against closed forms."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import normals_oracle as O  # noqa: E402


def test_plane_gives_its_normal_exactly():
    """z constant: the covariance's z row and column are exactly 0, so eigh returns (0, 0, 1) and l0 = 0 without rounding"""
    r = np.random.RandomState(1)
    p = np.concatenate([r.random_sample((300, 2)), np.full((300, 1), 2.0)], axis=1).astype(np.float32)
    res = O.normals(p, 16)
    assert res["ok"].all()
    assert np.array_equal(res["normal"], np.tile(np.float32([0, 0, 1]), (300, 1)))
    assert np.array_equal(res["variation"], np.zeros(300, np.float32))


def test_tilted_plane():
    """x + 2 y + 2 z = 3 sampled in float64 and rounded to fp32: off the plane by at most half an ulp per coordinate (6e-8 below 1), so
    over neighbourhoods about 0.1 wide the normal is (1, 2, 2) / 3 within 1e-5 and the variation below 1e-10"""
    r = np.random.RandomState(2)
    xy = r.random_sample((400, 2))
    p = np.concatenate([xy, ((3.0 - xy[:, 0] - 2.0 * xy[:, 1]) / 2.0)[:, None]], axis=1).astype(np.float32)
    res = O.normals(p, 16)
    want = np.float64([1, 2, 2]) / 3.0
    assert np.abs(res["normal"].astype(np.float64) - want).max() < 1e-5
    assert res["variation"].max() < 1e-10


def test_neighbours_are_the_stable_order_with_the_point_itself_first():
    p = O.lattice(5)                                            # massive ties
    idx = O.neighbors(p, 8)
    assert np.array_equal(idx[:, 0], np.arange(len(p)))         # d2 = 0: the point itself (no duplicates here)
    d2 = O.sqdist_rows(p, 0, len(p))
    for i in (0, 31, 62, 124):
        key = sorted((d2[i, j], j) for j in range(len(p)))[:8]
        assert [j for _, j in key] == list(idx[i])
    # fewer points than k: padded with -1
    assert np.array_equal(O.neighbors(p[:3], 4), np.int32([[0, 1, 2, -1], [1, 0, 2, -1], [2, 1, 0, -1]]))


def test_sphere_normals_are_radial_within_the_curvature_bound():
    """A point of the unit sphere at chord distance d from p lies d^2 / 2 below p's tangent plane.  With r the largest neighbour distance
    the heights h lie in [0, r^2 / 2], so sd(h) <= r^2 / 4 (Popoviciu).  Write the PCA normal as cos(t) z + sin(t) u, z radial, u a
    tangent unit vector: its variance n^T Cov n <= z^T Cov z = var(h), and by the triangle inequality for standard deviations
    sd(n . q) >= sin(t) sd(u . q) - cos(t) sd(h), hence sin(t) <= 2 sd(h) / sd(u . q) <= r^2 / (2 sqrt(lmin)), lmin the smallest
    eigenvalue of the neighbourhood's tangential 2x2 covariance."""
    p = O.sphere(4097)
    res = O.normals(p, 16)
    assert res["ok"].all()
    p64 = p.astype(np.float64)
    z = p64 / np.linalg.norm(p64, axis=1, keepdims=True)
    q = p64[res["idx"]] - p64[:, None, :]
    r = np.sqrt((q * q).sum(axis=2).max(axis=1))
    t = q - (q * z[:, None, :]).sum(axis=2, keepdims=True) * z[:, None, :]
    tc = t - t.mean(axis=1, keepdims=True)
    tcov = np.einsum("nki,nkj->nij", tc, tc) / 16.0             # rank 2 in the tangent plane: eigenvalues 0 <= lmin <= lmax
    lmin = np.linalg.eigvalsh(tcov)[:, 1]
    bound = np.minimum(1.0, r * r / (2.0 * np.sqrt(lmin)))
    sin_t = np.linalg.norm(np.cross(res["evec"], z), axis=1)
    assert (sin_t <= bound + 1e-6).all()                        # 1e-6: the fp32 points are off the sphere by 6e-8
    # the bound says something: 16 of 4097 points fill a cap of radius r with r^2 = 16 * 4 / 4097, and a disk of radius r has a
    # variance of r^2 / 4 per axis, so the bound is about r = 0.125; twice that is allowed for
    assert np.median(bound) < 2.0 * np.sqrt(64.0 / 4097.0)


def test_sign_rules():
    n = np.float32([[0.6, -0.8, 0.0], [-0.6, 0.0, 0.8], [0.5, 0.5, -np.sqrt(0.5)], [-np.sqrt(0.5), 0.5, 0.5], [-0.5, np.sqrt(0.5), -0.5],
                    [np.sqrt(0.5), -np.sqrt(0.5), 0.0], [-np.sqrt(0.5), np.sqrt(0.5), 0.0]])
    c = O.canonical_sign(n)
    lead = [1, 2, 2, 0, 1, 0, 0]                                # ties: the lowest axis
    for row, a in zip(c, lead):
        assert row[a] > 0 and abs(row[a]) == np.abs(row).max()
    assert np.array_equal(np.abs(c), np.abs(n))
    d = np.float64([[0, -1, 0], [0, 0, 1], [0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 1, 0], [1, 1, 0]])
    o = O.orient_sign(c, d)
    dots = np.einsum("ni,ni->n", o.astype(np.float64), d)
    assert (dots >= 0).all()
    for i in (2, 5, 6):                                         # a dot product of exactly 0 keeps the canonical sign
        assert dots[i] == 0 and np.array_equal(o[i], c[i])
    assert np.array_equal(o[0], -c[0]) and np.array_equal(o[4], -c[4])


def test_degenerate_neighbourhoods():
    two = O.normals(np.float32([[0, 0, 0], [1, 0, 0]]), 4)
    assert not two["ok"].any() and not two["normal"].any() and (two["variation"] == -1).all()
    same = O.normals(np.ones((6, 3), np.float32), 4)
    assert not same["ok"].any() and not same["normal"].any() and (same["variation"] == -1).all()


def test_viewpoint_mode():
    p = O.sphere(257, seed=3)
    out = O.normals(p, 8, 2, np.float32([0, 0, 0]))["normal"]                   # the viewpoint at the centre: inwards
    assert ((out.astype(np.float64) * p).sum(axis=1) < 0).all()
