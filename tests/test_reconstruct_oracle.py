"""CPU tests of tests/reconstruct_oracle.py, the numpy restatement the device is held to bit for bit (test_reconstruct_gpu.py): the
oracle must be a sound yardstick by itself.  Closedness is combinatorial: every directed edge occurs once and its reverse once.

Measured with this oracle (the conditions asserted below are the margins, not these figures):
  sphere(2048), h = 0.1, k = 8, support 1.5, band 1: V = 5682, F = 11360, 4954 active voxels, 6872 lattice vertices; closed, chi = 2,
      no unreferenced vertex; signed volume +0.31 % off 4 pi / 3; every vertex within 0.100 h of the unit sphere
  torus(2048), analytic normals: V = 6144, F = 12288, closed, chi = 0, volume 2.44453 against 2 pi^2 R r^2 = 2.41807 (+1.09 %)
  two_spheres(), h = 0.15: V = 5050, F = 10092, closed, chi = 4
  sphere(2048), h = 0.05: band 1 leaves 682 unpaired directed edges (chi = -61); band 2 is closed, chi = 2, V = 22706, F = 45408
  noisy_plane(), h = 0.05: open, no directed edge twice, chi = 1 (V = 2717, F = 5234)
  lattice_plane(), h = 1: f == 0 at 729 lattice vertices; 4056 of 5408 faces have zero area; finite, no directed edge twice
  far_ellipsoid(), h = 1e-3: closed, chi = 2, 69 zero-area faces of 4184
  one point, h = 0.25: 49 vertices, 72 faces
  torus with estimated, spanning-forest oriented normals: closed, chi = 0, V = 6156, F = 12312, volume +2.44621 (+1.16 %)
The slowest oracle run (sphere at h = 0.05, band 2) takes about 2 s; runs are shared through reconstruct_oracle.case_result."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reconstruct_oracle as R  # noqa: E402
import normals_oracle as NO  # noqa: E402


def mesh(name):
    r = R.case_result(name)
    return r["verts"], r["faces"], r


def test_sphere_is_a_closed_sphere():
    v, f, r = mesh("sphere")
    s = R.edge_stats(f)
    print("V %d F %d" % (len(v), len(f)))
    assert s["repeated"] == 0 and s["unpaired"] == 0
    assert R.euler(v, f) == 2 and R.unreferenced(v, f) == 0
    vol = R.volume(v, f)
    off = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).max() / 0.1
    print("volume %+.4f %% off, vertices within %.3f h" % (100 * (vol / (4 * np.pi / 3) - 1), off))
    assert vol > 0 and abs(vol / (4 * np.pi / 3) - 1) <= 0.02
    assert off <= 0.25
    assert f.dtype == np.int32 and v.dtype == np.float32 and f.min() >= 0 and f.max() == len(v) - 1


def test_torus_and_two_spheres_have_their_genus_and_components():
    v, f, _ = mesh("torus")
    assert R.closed(f) and R.euler(v, f) == 0
    print("torus volume %+.3f %% off" % (100 * (R.volume(v, f) / (2 * np.pi ** 2 * 0.35 ** 2) - 1)))
    assert abs(R.volume(v, f) / (2 * np.pi ** 2 * 0.35 ** 2) - 1) <= 0.02
    v, f, _ = mesh("two_spheres")
    assert R.closed(f) and R.euler(v, f) == 4


def test_a_voxel_below_the_spacing_leaves_holes_at_band_1_and_band_2_closes_them():
    """the documented limit and its remedy"""
    v, f, _ = mesh("sphere_fine_band1")
    s = R.edge_stats(f)
    print("band 1: %d unpaired directed edges" % s["unpaired"])
    assert s["repeated"] == 0 and s["unpaired"] > 0 and not R.closed(f)
    v, f, _ = mesh("sphere_fine_band2")
    assert R.closed(f) and R.euler(v, f) == 2


def test_an_open_surface():
    v, f, _ = mesh("noisy_plane")
    assert R.edge_stats(f)["repeated"] == 0 and R.euler(v, f) == 1


def test_exact_zeros_give_zero_area_faces_that_are_kept():
    v, f, r = mesh("lattice_plane")
    zeros, flat = int((r["f"] == 0).sum()), R.zero_area(v, f)
    print("f == 0 at %d lattice vertices, %d of %d faces have zero area" % (zeros, flat, len(f)))
    assert zeros >= 24 * 24                                   # a whole layer of the lattice
    assert np.isfinite(v).all() and R.edge_stats(f)["repeated"] == 0
    assert flat > 0 and flat < len(f)
    assert (r["f"][r["f"] == 0] >= 0).all() and R.unreferenced(v, f) == 0


def test_far_from_the_origin_the_mesh_stays_closed():
    """lattice indices near 10^6, fp32 lattice positions 6e-5 apart at h = 1e-3: vertices collapse, the connectivity does not"""
    v, f, _ = mesh("far_ellipsoid")
    print("%d zero-area faces of %d" % (R.zero_area(v, f), len(f)))
    assert R.closed(f) and R.euler(v, f) == 2 and np.isfinite(v).all()


def test_one_point_gives_a_small_open_patch():
    v, f, _ = mesh("one_point")
    print("V %d F %d" % (len(v), len(f)))
    assert len(v) > 0 and len(f) > 0 and np.isfinite(v).all() and R.edge_stats(f)["repeated"] == 0
    assert np.abs(v[:, 2] - np.float32(0.3)).max() <= 1e-6    # the tangent plane of the one point


def test_from_estimated_normals():
    v, f, _ = mesh("estimated_torus")
    assert R.closed(f) and R.euler(v, f) == 0
    vol = R.volume(v, f)                                      # negative if the anchor rule had oriented the component inwards
    print("volume %+.5f" % vol)
    assert abs(abs(vol) / (2 * np.pi ** 2 * 0.35 ** 2) - 1) <= 0.02


def test_signed_distance_has_the_sign_of_the_side():
    p = NO.sphere(2048)
    d = NO.sphere(500, seed=5).astype(np.float64)
    # The tangent plane of a neighbour at angle t passes 1 - cos t ~ t^2 / 2 inside the sphere above the query.  The 8th neighbour of
    # 2048 points lies near t = sqrt(8 * 4 / 2048) = 0.125, so the function's zero sits up to 0.008 inside: delta starts at 0.02
    for delta in (0.2, 0.05, 0.02):
        out = R.signed_distance((d * (1 + delta)).astype(np.float32), p, p)
        inn = R.signed_distance((d * (1 - delta)).astype(np.float32), p, p)
        assert (out > 0).all() and (inn < 0).all(), delta
    one = R.signed_distance(np.float32([[0, 0, 2], [0, 0, -1]]), np.float32([[0, 0, 0]]), np.float32([[0, 0, 1]]), k=8)
    assert one.tolist() == [2.0, -1.0]                        # k' = 1: the tangent plane of the one point
    same = R.signed_distance(np.float32([[1, 2, 3.5]]), np.tile(np.float32([[1, 2, 3]]), (5, 1)), np.tile(np.float32([[0, 0, 2]]), (5, 1)), k=4)
    assert same.tolist() == [1.0]                             # equidistant neighbours: every weight is 0, normals are not normalised


def test_the_case_table_is_consistent_and_is_the_one_the_kernels_hold():
    T = R.case_table()
    for t in range(6):
        for m in range(16):
            flipped = T[t][15 - m]                            # the complementary signs: the same triangles, reversed
            assert sorted(tuple(sorted(tri)) for tri in T[t][m]) == sorted(tuple(sorted(tri)) for tri in flipped)
            for tri in T[t][m]:
                assert any(tri == (o[i], o[(i + 2) % 3], o[(i + 1) % 3]) for o in flipped for i in range(3))
    text = open(os.path.join(ROOT, "dis-pu_amd", "csrc", "reconstruct.hip")).read()
    body = re.search(r"kTetCase\[6\]\[16\]\[7\] = \{(.*?)\};", text, flags=re.S).group(1)
    have = np.array([int(x) for x in re.findall(r"\d+", body)], np.uint8).reshape(6, 16, 7)
    assert np.array_equal(have, R.case_bytes())
    tet = re.search(r"kTet\[6\]\[4\] = \{(.*?)\};", text, flags=re.S).group(1)
    assert [int(x) for x in re.findall(r"\d+", tet)] == [b for row in R.tets() for b in row]


def test_range_and_vertex_limits_are_refused():
    with pytest.raises(ValueError, match="voxel"):
        R.reconstruct(np.float32([[1000, 0, 0]]), np.float32([[0, 0, 1]]), 1e-4)
    p = NO.sphere(2048)
    with pytest.raises(ValueError, match="max_vertices"):
        R.reconstruct(p, p, 0.1, max_vertices=100)
    edge = np.float32([[(R.BIAS - 1) * 0.5, 0, -(R.BIAS - 1) * 0.5]])      # the last index band 1 admits, on both sides
    r = R.reconstruct(edge, np.float32([[0, 0, 1]]), 0.5)
    assert len(r["faces"]) > 0 and np.isfinite(r["verts"]).all()
    with pytest.raises(ValueError, match="voxel"):
        R.reconstruct(edge, np.float32([[0, 0, 1]]), 0.5, band=2)
