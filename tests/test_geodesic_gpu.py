"""GPU tests of the exact geodesic disks (csrc/geodesic.hip through dis-pu_amd/mesh.py and evaluate.py) against the float64 oracle of
tests/geodesic_oracle.py and closed forms: the fixtures of tests/geodesic_fixtures.py, seeds on the PU-GAN test meshes, the full
1000-seed membership, a planar mesh, a subdivided sphere, the arena rerun path and the evaluator's geodesic mode."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geodesic_fixtures as GF  # noqa: E402
import geodesic_oracle as GO  # noqa: E402
import mesh_oracle as MO  # noqa: E402

import dispu_amd  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SHAPES = ["Icosahedron", "fandisk"]


@pytest.fixture(scope="module")
def pugan(golden_dir, tmp_path_factory):
    return MO.extract_pugan(golden_dir, str(tmp_path_factory.mktemp("pugan")))


@pytest.fixture(scope="module")
def meshes(dev, pugan):
    from dispu_amd import mesh as M
    return {s: M.Mesh.from_off(os.path.join(pugan, s + ".off"), dev) for s in SHAPES}


@pytest.fixture(scope="module")
def outputs(dev, pugan, meshes):
    """per shape: the network's 8192 points projected onto the mesh, 1000 seeds and the radii"""
    from dispu_amd import mesh as M
    out = {}
    for s in SHAPES:
        mesh = meshes[s]
        pts = torch.from_numpy(np.loadtxt(os.path.join(pugan, s + "_X4.xyz"))[:, :3].astype(np.float32)).to(dev)
        _, proj, face = M.point_to_mesh(pts, mesh)
        fid, bary = M.sample_surface_seeds(mesh, 1000, seed=0)
        out[s] = (proj, face, fid, bary, M.disk_radii(mesh))
    return out


def _rows(off, mem):
    off, mem = off.cpu().numpy(), mem.cpu().numpy()
    return [mem[off[k]:off[k + 1]] for k in range(off.shape[0] - 1)]


def _dense(cand_off, cand, dist, S, n):
    """CSR distances -> [S, n] with +inf where a point is not a candidate"""
    o, c, d = cand_off.cpu().numpy(), cand.cpu().numpy(), dist.cpu().numpy()
    out = np.full((S, n), np.inf)
    for i in range(S):
        out[i, c[o[i]:o[i + 1]]] = d[o[i]:o[i + 1]]
    return out


@pytest.mark.parametrize("name", sorted(GF.CASES))
def test_closed_form_fixtures(dev, name):
    """The kernel on the fixture as the device sees it (Mesh keeps f32 vertices, targets are f32) against the oracle on those same
    inputs to 1e-9 relative.  The closed form holds for the fp64 fixture (tests/test_geodesic.py checks the oracle on it to 1e-9);
    here it is only a sanity check, at 1e-5 relative: the f32 rounding of the vertices and targets (2^-24 relative) moves the
    distances by about 1e-7."""
    from dispu_amd import mesh as M
    v, f, (sf, sb), t, tf, exp = GF.CASES[name]()
    mesh = M.Mesh(v, f, dev)
    t32 = t.astype(np.float32)
    pts = torch.from_numpy(t32).to(dev)
    pf = torch.from_numpy(tf.astype(np.int32)).to(dev)
    maxd = 4.0
    off, cand, dist = M.geodesic_distances(mesh, [sf], [sb], pts, pf, maxd)
    got = _dense(off, cand, dist, 1, t.shape[0])[0]
    ref = GO.geodesic(mesh.verts, mesh.faces, sf, sb, t32, tf, maxd)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=0)
    np.testing.assert_allclose(got, exp, rtol=1e-5, atol=0)


def test_folded_is_above_the_chord(dev):
    from dispu_amd import mesh as M
    v, f, (sf, sb), t, tf, exp = GF.folded_case(70.0)
    mesh = M.Mesh(v, f, dev)
    off, cand, dist = M.geodesic_distances(mesh, [sf], [sb], torch.from_numpy(t.astype(np.float32)).to(dev),
                                           torch.from_numpy(tf.astype(np.int32)).to(dev), 4.0)
    got = _dense(off, cand, dist, 1, t.shape[0])[0]
    chord = np.linalg.norm(t - mesh.surface_points([sf], [sb]), axis=1)
    across = t[:, 2] > 1e-3                                           # targets on the other sheet
    assert across.any() and np.all(got[across] > chord[across] * (1 + 1e-3))


@pytest.mark.parametrize("shape", SHAPES)
def test_pugan_seeds_against_oracle(dev, meshes, outputs, shape):
    from dispu_amd import mesh as M
    mesh = meshes[shape]
    proj, face, fid, bary, radii = outputs[shape]
    sel = np.arange(0, 1000, 125)                                    # 8 seeds
    maxd = float(radii.max())
    off, cand, dist = M.geodesic_distances(mesh, fid[sel], bary[sel], proj, face, maxd)
    got = _dense(off, cand, dist, sel.size, proj.shape[0])
    P, Fq = proj.cpu().numpy(), face.cpu().numpy()
    surf = GO.Surface(mesh.verts, mesh.faces)
    seeds = mesh.surface_points(fid[sel], bary[sel])
    for r, i in enumerate(sel):
        near = np.nonzero(np.linalg.norm(P.astype(np.float64) - seeds[r], axis=1) <= maxd * 1.001)[0]
        ref = GO.geodesic(mesh.verts, mesh.faces, fid[i], bary[i], P[near], Fq[near], maxd, surface=surf)
        g = got[r, near]
        fin = np.isfinite(ref) & (ref < maxd * (1 - 1e-7))
        np.testing.assert_allclose(g[fin], ref[fin], rtol=1e-9, atol=0)
        # membership: index-exact outside the 1e-7 band around every radius
        for rj in radii.astype(np.float64):
            clear = np.abs(ref - rj) > 1e-7 * rj
            assert np.array_equal((g <= rj)[clear], (ref <= rj)[clear])
    offs, mem = M.geodesic_disk_members(mesh, fid[sel], bary[sel], proj, face, radii)
    rows = _rows(offs, mem)
    for r in range(sel.size):
        for j, rj in enumerate(radii.astype(np.float64)):
            assert np.array_equal(rows[r * 2 + j], np.nonzero(got[r] <= rj)[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_full_seeds_subset_and_deterministic(dev, meshes, outputs, shape):
    from dispu_amd import mesh as M
    mesh = meshes[shape]
    proj, face, fid, bary, radii = outputs[shape]
    seeds = torch.from_numpy(mesh.surface_points(fid, bary).astype(np.float32)).to(dev)
    eo, em = M.disk_members(seeds, proj, radii)
    go, gm = M.geodesic_disk_members(mesh, fid, bary, proj, face, radii)
    go2, gm2 = M.geodesic_disk_members(mesh, fid, bary, proj, face, radii)
    assert torch.equal(go, go2) and torch.equal(gm, gm2)
    E, G = _rows(eo, em), _rows(go, gm)
    assert len(G) == 2000
    strict = 0
    for e, g in zip(E, G):
        assert np.all(np.diff(g) > 0)
        assert np.isin(g, e).all()
        strict += len(e) - len(g)
    if shape == "fandisk":
        assert strict > 0
    off, cand, dist = M.geodesic_distances(mesh, fid, bary, proj, face, float(radii.max()))
    off2, cand2, dist2 = M.geodesic_distances(mesh, fid, bary, proj, face, float(radii.max()))
    assert torch.equal(dist, dist2) and torch.equal(cand, cand2)


def test_tiny_arena_reruns_to_the_same_result(dev, meshes, outputs):
    from dispu_amd import mesh as M
    mesh = meshes["fandisk"]
    proj, face, fid, bary, radii = outputs["fandisk"]
    sel = slice(0, 64)
    a = M.geodesic_distances(mesh, fid[sel], bary[sel], proj, face, float(radii.max()))
    b = M.geodesic_distances(mesh, fid[sel], bary[sel], proj, face, float(radii.max()), arena=8)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_planar_mesh_geodesic_equals_euclidean(dev):
    from dispu_amd import mesh as M
    v, f = GF.grid(40, 40, jitter=0.3, seed=5)
    mesh = M.Mesh(v, f, dev)
    rng = np.random.default_rng(6)
    pts = np.concatenate([rng.random((6000, 2)), np.zeros((6000, 1))], 1).astype(np.float32)
    p = torch.from_numpy(pts).to(dev)
    _, proj, face = M.point_to_mesh(p, mesh)
    fid, bary = M.sample_surface_seeds(mesh, 200, seed=2)
    radii = M.disk_radii(mesh)
    seeds = mesh.surface_points(fid, bary)
    eo, em = M.disk_members(torch.from_numpy(seeds.astype(np.float32)).to(dev), proj, radii)
    go, gm = M.geodesic_disk_members(mesh, fid, bary, proj, face, radii)
    P = proj.cpu().numpy().astype(np.float64)
    for k, (e, g) in enumerate(zip(_rows(eo, em), _rows(go, gm))):
        i, rj = k // 2, float(radii[k % 2])
        d = np.linalg.norm(P - seeds[i], axis=1)
        band = np.nonzero(np.abs(d - rj) <= 1e-5 * rj)[0]           # f32 Euclidean test vs fp64 geodesic: only the band may differ
        assert np.array_equal(np.setdiff1d(e, band), np.setdiff1d(g, band))


def test_icosphere_follows_the_great_circle(dev):
    """Vertices on the sphere of radius R; every face lies in the shell between R cos(phi) and R, phi the largest angle between a
    face's normal and one of its vertices.  A surface path outside the ball of radius R cos(phi) is at least R cos(phi) * alpha long
    (the nearest-point map onto a convex ball shortens curves), alpha the angle between the ends; the central projection of the arc
    of angle alpha onto the faces is a surface path of length at most R alpha / cos(phi)^2 (the gnomonic projection onto a plane at
    distance h <= R stretches arcs of the sphere by at most 1 / cos^2).  So R a cos(phi) <= d <= R a / cos(phi)^2."""
    from dispu_amd import mesh as M, synth
    R = 0.8
    v, f = synth.icosphere(5, radius=R)
    mesh = M.Mesh(v, f, dev)
    tv = mesh.verts[mesh.faces].astype(np.float64)
    n = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cos_phi = (np.einsum("fc,fkc->fk", n, tv) / np.linalg.norm(tv, axis=2)).min()
    rng = np.random.default_rng(9)
    g = rng.standard_normal((20000, 3))
    pts = torch.from_numpy((g / np.linalg.norm(g, axis=1, keepdims=True) * R).astype(np.float32)).to(dev)
    _, proj, face = M.point_to_mesh(pts, mesh)
    fid, bary = M.sample_surface_seeds(mesh, 48, seed=3)
    off, cand, dist = M.geodesic_distances(mesh, fid, bary, proj, face, 0.3)
    o, c, d = off.cpu().numpy(), cand.cpu().numpy(), dist.cpu().numpy()
    P = proj.cpu().numpy().astype(np.float64)
    seeds = mesh.surface_points(fid, bary)
    checked = 0
    for i in range(fid.shape[0]):
        q, di = c[o[i]:o[i + 1]], d[o[i]:o[i + 1]]
        fin = np.isfinite(di)
        u = P[q[fin]] / np.linalg.norm(P[q[fin]], axis=1, keepdims=True)
        s = seeds[i] / np.linalg.norm(seeds[i])
        alpha = np.arccos(np.clip(u @ s, -1, 1))
        assert np.all(di[fin] >= R * alpha * cos_phi * (1 - 1e-9))
        assert np.all(di[fin] <= R * alpha / cos_phi ** 2 * (1 + 1e-9) + 1e-12)
        chord = np.linalg.norm(P[q[fin]] - seeds[i], axis=1)
        assert np.all(di[fin] >= chord * (1 - 1e-12))
        checked += fin.sum()
    assert checked > 48 * 100


def test_non_manifold_mesh_raises(dev):
    from dispu_amd import mesh as M
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)
    mesh = M.Mesh(v, f, dev)
    pts = torch.tensor([[0.2, 0.2, 0.0]], dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="non-manifold"):
        M.mesh_metrics(pts, mesh, seeds=4, disks="geodesic")
    M.mesh_metrics(pts.repeat(8, 1), mesh, seeds=4)                  # Euclidean disks do not need the tables


def test_evaluate_pair_geodesic(dev, pugan, meshes):
    from dispu_amd.evaluate import evaluate_pair
    pred = np.loadtxt(os.path.join(pugan, "fandisk_X4.xyz"))[:, :3]
    gt = pred[::2]
    base = evaluate_pair(pred, gt, mesh=meshes["fandisk"])
    eu = evaluate_pair(pred, gt, mesh=meshes["fandisk"], disks="euclidean")
    geo = evaluate_pair(pred, gt, mesh=meshes["fandisk"], disks="geodesic")
    assert base == eu and base["uniformity_mode"] == "euclidean"
    assert geo["uniformity_mode"] == "geodesic" and geo["CD"] == base["CD"] and geo["p2f avg"] == base["p2f avg"]
    assert np.isfinite(geo["uniform_0"]) and np.isfinite(geo["uniform_1"])
    assert (geo["uniform_0"], geo["uniform_1"]) != (base["uniform_0"], base["uniform_1"])
    with pytest.raises(ValueError, match="disks"):
        evaluate_pair(pred, gt, mesh=meshes["fandisk"], disks="heat")


def test_evaluate_dirs_geodesic_round_trip(dev, pugan, tmp_path):
    import shutil
    from dispu_amd import mesh as M
    from dispu_amd.evaluate import evaluate_dirs
    for d in ("pred", "gt", "mesh"):
        (tmp_path / d).mkdir()
    for s in SHAPES:
        pts = np.loadtxt(os.path.join(pugan, s + "_X4.xyz"))[:, :3]
        np.savetxt(tmp_path / "pred" / (s + ".xyz"), pts, fmt="%.6f")
        np.savetxt(tmp_path / "gt" / (s + ".xyz"), pts[::-1], fmt="%.6f")
        shutil.copy(os.path.join(pugan, s + ".off"), tmp_path / "mesh" / (s + ".off"))
    eu = evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), csv_name="eu.csv", mesh_dir=str(tmp_path / "mesh"))
    rows = evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), mesh_dir=str(tmp_path / "mesh"), write_cgal_files=True,
                         disks="geodesic")
    assert all(r["uniformity_mode"] == "geodesic" for r in rows)
    assert any(a["uniform_1"] != b["uniform_1"] for a, b in zip(eu, rows))
    for s, r in zip(sorted(SHAPES), rows):
        c = M.read_cgal_files(str(tmp_path / "pred" / (s + ".xyz")))
        assert c["offsets"].shape[0] == 2001
    back = evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), csv_name="again.csv", use_cgal_files=True)
    for a, b in zip(rows, back):
        assert b["uniformity_mode"] == "cgal_files"
        for k in ("p2f avg", "p2f std", "uniform_0", "uniform_1"):
            assert a[k] == b[k], (k, a[k], b[k])
