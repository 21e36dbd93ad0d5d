"""CPU tests of the exact geodesic disks: the host tables of dis-pu_amd/mesh.py (twins, angle sums, pseudo-sources, fans, the
non-manifold check) and the float64 oracle of tests/geodesic_oracle.py against closed forms (tests/geodesic_fixtures.py).
No kernel runs here."""
import math
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geodesic_fixtures as GF  # noqa: E402
import geodesic_oracle as GO  # noqa: E402
import mesh_oracle as MO  # noqa: E402

import dispu_amd  # noqa: E402,F401
from dispu_amd import mesh as M  # noqa: E402


@pytest.fixture(scope="module")
def pugan(golden_dir, tmp_path_factory):
    return MO.extract_pugan(golden_dir, str(tmp_path_factory.mktemp("pugan")))


def _angle_sums(v, f):
    v = v.astype(np.float64)
    out = np.zeros(v.shape[0])
    for j in range(3):
        p, q, r = v[f[:, j]], v[f[:, (j + 1) % 3]], v[f[:, (j + 2) % 3]]
        a, b = q - p, r - p
        out += np.bincount(f[:, j], np.arccos(np.clip(np.sum(a * b, 1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1), -1, 1)),
                           minlength=v.shape[0])
    return out


@pytest.mark.parametrize("name", ["Icosahedron", "fandisk"])
def test_tables_on_pugan(pugan, name):
    v, f = M.load_off(os.path.join(pugan, name + ".off"))
    T = M.geodesic_tables(v, f)
    F = f.shape[0]
    tw = T["twin"].reshape(-1)
    assert np.all(tw >= 0)                                              # closed meshes: every edge has its twin
    assert np.array_equal(tw[tw], np.arange(3 * F))                    # exactly one, and it points back
    fa, ka = np.arange(3 * F) // 3, np.arange(3 * F) % 3
    fb, kb = tw // 3, tw % 3
    assert np.all(fa != fb)
    assert np.array_equal(f[fa, ka], f[fb, (kb + 1) % 3]) and np.array_equal(f[fa, (ka + 1) % 3], f[fb, kb])
    np.testing.assert_allclose(T["angle_sum"], _angle_sums(v, f), rtol=1e-12, atol=1e-12)
    assert np.array_equal(T["pseudo"] == 1, T["angle_sum"] >= 2 * np.pi)
    if name == "fandisk":
        assert abs(T["angle_sum"].max() / np.pi - 2.75) < 0.01
    # edge frames: L, cx, cy reproduce the third vertex's distances
    g = T["edge_geo"]
    v64 = v.astype(np.float64)
    for k in range(3):
        a, b, c = v64[f[:, k]], v64[f[:, (k + 1) % 3]], v64[f[:, (k + 2) % 3]]
        np.testing.assert_allclose(g[:, k, 0], np.linalg.norm(b - a, axis=1), rtol=1e-14)
        np.testing.assert_allclose(np.hypot(g[:, k, 1], g[:, k, 2]), np.linalg.norm(c - a, axis=1), rtol=1e-12)
        np.testing.assert_allclose(np.hypot(g[:, k, 1] - g[:, k, 0], g[:, k, 2]), np.linalg.norm(c - b, axis=1), rtol=1e-10)
    assert np.all(g[:, :, 2] > 0)
    # fans: every corner once, each under its own vertex
    fan, off = T["fan"], T["fan_off"]
    assert np.array_equal(np.sort(fan), np.arange(3 * F))
    for vv in (0, 17, v.shape[0] - 1):
        c = fan[off[vv]:off[vv + 1]]
        assert np.all(f[c // 3, c % 3] == vv)


def test_tables_boundary_and_non_manifold():
    v, f = GF.grid(3, 2)
    T = M.geodesic_tables(v, f)
    assert (T["twin"] < 0).sum() == 2 * (3 + 2)
    assert np.array_equal(T["boundary"], (v[:, 0] == 0) | (v[:, 0] == 1) | (v[:, 1] == 0) | (v[:, 1] == 1))
    assert np.all(T["pseudo"][T["boundary"]] == 1)
    nv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    nf = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)
    with pytest.raises(ValueError, match="non-manifold"):
        M.geodesic_tables(nv, nf)
    # the Mesh method raises before it copies anything to a device
    with pytest.raises(ValueError, match="non-manifold"):
        M.Mesh.geodesic_tables(types.SimpleNamespace(verts=nv, faces=nf))
    with pytest.raises(ValueError, match="disks"):
        M.mesh_metrics(None, None, disks="heat")


@pytest.mark.parametrize("name", sorted(GF.CASES))
def test_oracle_closed_forms(name):
    v, f, (sf, sb), t, tf, exp = GF.CASES[name]()
    d = GO.geodesic(v, f, sf, sb, t, tf, 10.0)
    np.testing.assert_allclose(d, exp, rtol=1e-9, atol=0)


def test_fixtures_cover_their_cases():
    # folded sheets: the geodesic is strictly above the chord for targets across the fold
    v, f, (sf, sb), t, tf, exp = GF.folded_case(70.0)
    s = sb @ v[f[sf]]
    across = t[:, 2] > 1e-3
    assert across.any() and np.all(exp[across] > np.linalg.norm(t[across] - s, axis=1) * (1 + 1e-3))
    # cones: both the straight unrolled line and the path over the apex occur, on convex, saddle and open fans
    for theta, closed in ((1.5 * math.pi, True), (2.5 * math.pi, True), (3 * math.pi, True), (1.5 * math.pi, False)):
        v, f, (sf, sb), t, tf, exp = GF.cone_case(theta, closed=closed)
        T = M.geodesic_tables(v, f)
        assert abs(T["angle_sum"][0] - theta) < 1e-9
        assert bool(T["pseudo"][0]) == (theta >= 2 * math.pi or not closed)
        s = sb @ v[f[sf]]
        through_apex = np.abs(exp - (np.linalg.norm(s) + np.linalg.norm(t, axis=1))) < 1e-12
        if theta > 2 * math.pi:
            assert through_apex.any() and (~through_apex).any()
    # seeds exactly on an edge and on a vertex
    assert (GF.seed_on_edge_case()[2][1] == 0).sum() == 1
    assert (GF.seed_on_vertex_case()[2][1] == 0).sum() == 2


def test_oracle_pruning_keeps_distances():
    """the priority-queue oracle with max_dist: distances below it do not change when max_dist grows"""
    v, f, (sf, sb), t, tf, exp = GF.cone_case(2.5 * math.pi)
    a = GO.geodesic(v, f, sf, sb, t, tf, 0.2)
    b = GO.geodesic(v, f, sf, sb, t, tf, 10.0)
    keep = b <= 0.2
    assert keep.any() and np.array_equal(a[keep], b[keep]) and np.all(np.isinf(a[~keep]))
