"""GPU tests of the evaluator's mesh metrics (csrc/mesh_eval.hip through dis-pu_amd/mesh.py and evaluate.py) against the float64
oracle of tests/mesh_oracle.py: P2F on the PU-GAN test meshes and constructed points, pruned vs brute force, Euclidean disk
membership, uniformity, and the seven-column evaluate_dirs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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


def _check_p2f(mesh, pts, dev):
    from dispu_amd import mesh as M
    d, q, f = M.point_to_mesh(torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev), mesh)
    d, q, f = d.cpu().numpy(), q.cpu().numpy(), f.cpu().numpy()
    rd, rq, rf, gap = MO.point_to_mesh(pts.astype(np.float32), mesh.verts, mesh.faces)
    assert np.abs(d - rd).max() <= 2e-6
    clear = gap > 1e-6
    assert np.linalg.norm(q[clear] - rq[clear], axis=1).max() <= 1e-5
    assert np.array_equal(f[clear], rf[clear])
    # proj is a point of the reported face, and dist its distance
    assert np.abs(np.linalg.norm(pts.astype(np.float64) - q, axis=1) - d).max() <= 2e-6
    return d, clear


@pytest.mark.parametrize("shape", SHAPES)
def test_p2f_network_outputs(dev, pugan, meshes, shape):
    pts = np.loadtxt(os.path.join(pugan, shape + "_X4.xyz"))[:, :3]
    assert pts.shape == (8192, 3)
    _, clear = _check_p2f(meshes[shape], pts, dev)
    assert clear.mean() > 0.9


@pytest.mark.parametrize("n", [1, 63, 65, 8193])
def test_p2f_constructed_points(dev, meshes, n):
    mesh = meshes["fandisk"]
    rng = np.random.default_rng(n)
    tv = mesh.verts[mesh.faces].astype(np.float64)
    nrm = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    kinds = rng.integers(0, 6, n)
    fid = rng.integers(0, mesh.num_faces, n)
    b = rng.random((n, 3)) + 0.05
    b /= b.sum(axis=1, keepdims=True)
    on = np.einsum("nk,nkc->nc", b, tv[fid])
    pts = np.where((kinds == 0)[:, None], mesh.verts[mesh.faces[fid, 0]], on)                               # on a vertex
    pts = np.where((kinds == 1)[:, None], 0.5 * (tv[fid, 0] + tv[fid, 1]), pts)                               # on an edge
    off = rng.uniform(0.001, 0.05, n)[:, None] * nrm[fid]
    pts = np.where((kinds == 2)[:, None], on + off, pts)                                                      # above
    pts = np.where((kinds == 3)[:, None], on - off, pts)                                                      # below
    far = rng.standard_normal((n, 3))
    pts = np.where((kinds == 4)[:, None], 3.0 * far / np.linalg.norm(far, axis=1, keepdims=True), pts)       # far away
    d, _ = _check_p2f(mesh, pts, dev)                                                                         # kind 5: interior
    surf = np.isin(kinds, [0, 1, 5])
    assert np.all(d[surf] <= 1e-6)


def test_p2f_surface_samples(dev, meshes):
    from dispu_amd import mesh as M
    for mesh in meshes.values():
        fid, bary = M.sample_surface_seeds(mesh, 4096, seed=11)
        pts = torch.from_numpy(mesh.surface_points(fid, bary).astype(np.float32)).to(dev)
        d, _, _ = M.point_to_mesh(pts, mesh)
        assert float(d.max()) <= 1e-6


@pytest.mark.parametrize("which", ["Icosahedron", "fandisk", "sphere"])
def test_p2f_pruned_equals_brute_force(dev, pugan, meshes, which):
    from dispu_amd import mesh as M, synth
    if which == "sphere":
        v, f = synth.icosphere(7, radius=0.8)
        mesh = M.Mesh(v, f, dev)
        assert mesh.num_faces >= 300000
        rng = np.random.default_rng(2)
        g = rng.standard_normal((8192, 3))
        pts = (g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0.7, 0.9, (8192, 1))).astype(np.float32)
    else:
        mesh = meshes[which]
        pts = np.loadtxt(os.path.join(pugan, which + "_X4.xyz"))[:, :3].astype(np.float32)
    p = torch.from_numpy(pts).to(dev)
    a = M.point_to_mesh(p, mesh)
    b = M.point_to_mesh(p, mesh, brute_force=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("shape", SHAPES)
def test_disk_membership_index_exact(dev, pugan, meshes, shape):
    from dispu_amd import mesh as M
    mesh = meshes[shape]
    pred = torch.from_numpy(np.loadtxt(os.path.join(pugan, shape + "_X4.xyz"))[:, :3].astype(np.float32)).to(dev)
    _, proj, _ = M.point_to_mesh(pred, mesh)
    fid, bary = M.sample_surface_seeds(mesh, 200, seed=4)
    seeds = mesh.surface_points(fid, bary).astype(np.float32)
    radii = np.concatenate([M.disk_radii(mesh), np.float32([10.0, 0.0])])     # + every point, + none (no projected point is a seed)
    off, mem = M.disk_members(torch.from_numpy(seeds).to(dev), proj, radii)
    off, mem = off.cpu().numpy(), mem.cpu().numpy()
    ref = MO.disk_members_fp32(seeds, proj.cpu().numpy(), radii)
    assert off.shape[0] == len(ref) + 1 and off[0] == 0
    for k, r in enumerate(ref):
        assert np.array_equal(mem[off[k]:off[k + 1]], r), k
    R = len(radii)
    assert all(off[i * R + 3] - off[i * R + 2] == 8192 for i in range(200))
    assert all(off[i * R + 4] == off[i * R + 3] for i in range(200))


@pytest.mark.parametrize("shape", SHAPES)
def test_uniformity_matches_oracle_and_repeats(dev, pugan, meshes, shape):
    from dispu_amd import mesh as M
    mesh = meshes[shape]
    pred = torch.from_numpy(np.loadtxt(os.path.join(pugan, shape + "_X4.xyz"))[:, :3].astype(np.float32)).to(dev)
    r1 = M.mesh_metrics(pred, mesh, seeds=1000, seed=0)
    r2 = M.mesh_metrics(pred, mesh, seeds=1000, seed=0)
    assert np.array_equal(r1["uniform"], r2["uniform"]) and r1["p2f avg"] == r2["p2f avg"] and r1["p2f std"] == r2["p2f std"]
    off, mem = r1["offsets"].cpu().numpy(), r1["members"].cpu().numpy()
    disks = [mem[off[k]:off[k + 1]] for k in range(off.shape[0] - 1)]
    ref = MO.analyze_uniform(disks, r1["radii"].astype(np.float64), r1["proj"].cpu().numpy())
    assert np.all(np.isfinite(ref))
    np.testing.assert_allclose(r1["uniform"], ref, rtol=1e-4)
    d = r1["dist"].cpu().numpy().astype(np.float64)
    assert abs(r1["p2f avg"] - d.mean()) <= 1e-12 + 1e-9 * d.mean() and abs(r1["p2f std"] - d.std()) <= 1e-9 * d.std()


def test_uniformity_large_and_skipped_disks(dev):
    from dispu_amd import mesh as M
    rng = np.random.default_rng(8)
    pts = rng.random((3000, 3)).astype(np.float32)
    pts[7] = pts[3]                                                    # a duplicate: its nearest other member is at 0
    rows = [np.arange(3000), np.arange(4), np.sort(rng.choice(3000, 700, replace=False)), np.arange(2)]   # S = 2, R = 2
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)).to(dev)
    mem = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(dev)
    radii, pct = np.array([0.9, 0.05]), np.array([0.5, 0.001])
    got = M.uniformity(torch.from_numpy(pts).to(dev), off, mem, radii, pct)
    ref = MO.analyze_uniform(rows, radii, pts, pct)
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-4)
    assert np.isnan(got[1]) and np.isnan(ref[1])


def test_fps_subsample_is_more_uniform(dev, meshes):
    from dispu_amd import mesh as M
    import dispu_amd.tf_sampling as S
    mesh = meshes["Icosahedron"]
    fid, bary = M.sample_surface_seeds(mesh, 32768, seed=21)
    dense = torch.from_numpy(mesh.surface_points(fid, bary).astype(np.float32)).to(dev)
    idx = S.farthest_point_sample(8192, dense.reshape(1, -1, 3))[0].long()
    fps = dense[idx].contiguous()
    iid = dense[:8192].contiguous()
    u_fps = M.mesh_metrics(fps, mesh, seeds=1000, seed=1)["uniform"]
    u_iid = M.mesh_metrics(iid, mesh, seeds=1000, seed=1)["uniform"]
    assert np.all(u_fps < u_iid), (u_fps, u_iid)


def test_evaluate_pair_with_mesh(dev, pugan, meshes):
    from dispu_amd.evaluate import evaluate_pair
    pred = np.loadtxt(os.path.join(pugan, "fandisk_X4.xyz"))[:, :3]
    gt = np.loadtxt(os.path.join(pugan, "fandisk_X4.xyz"))[::2, :3]
    plain = evaluate_pair(pred, gt)
    r = evaluate_pair(pred, gt, mesh=meshes["fandisk"])
    assert set(plain) == {"CD", "hausdorff", "cd_forward", "cd_backward"}
    assert r["CD"] == plain["CD"] and r["uniformity_mode"] == "euclidean"
    assert 0 < r["p2f avg"] < 0.05 and r["p2f std"] > 0 and np.isfinite(r["uniform_0"]) and np.isfinite(r["uniform_1"])


def test_evaluate_dirs_with_meshes(dev, pugan, tmp_path):
    import shutil
    from dispu_amd.evaluate import evaluate_dirs
    for d in ("pred", "gt", "mesh"):
        (tmp_path / d).mkdir()
    for s in SHAPES:
        pts = np.loadtxt(os.path.join(pugan, s + "_X4.xyz"))[:, :3]
        np.savetxt(tmp_path / "pred" / (s + ".xyz"), pts, fmt="%.6f")
        np.savetxt(tmp_path / "gt" / (s + ".xyz"), pts[::-1], fmt="%.6f")
        shutil.copy(os.path.join(pugan, s + ".off"), tmp_path / "mesh" / (s + ".off"))
    rows = evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), mesh_dir=str(tmp_path / "mesh"), write_cgal_files=True)
    lines = (tmp_path / "pred" / "evaluation.csv").read_text().strip().splitlines()
    assert lines[0] == "name,CD,hausdorff,p2f avg,p2f std,uniform_0,uniform_1" and len(lines) == 4
    assert lines[-1].startswith("avg,") and "-" not in lines[-1].split(",")
    assert all(r["uniformity_mode"] == "euclidean" for r in rows)
    for s in SHAPES:
        assert os.path.isfile(tmp_path / "pred" / (s + "_disk_idx.txt"))
    back = evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), csv_name="again.csv", use_cgal_files=True)
    for a, b in zip(rows, back):
        assert b["uniformity_mode"] == "cgal_files"
        for k in ("p2f avg", "p2f std", "uniform_0", "uniform_1"):
            assert a[k] == b[k], (k, a[k], b[k])
    assert (tmp_path / "pred" / "again.csv").read_text().strip().splitlines()[-1] == lines[-1]
    # without mesh_dir: the CD / hausdorff CSV of before
    evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), csv_name="plain.csv")
    plain = (tmp_path / "pred" / "plain.csv").read_text().strip().splitlines()
    assert plain[0] == "name,CD,hausdorff" and len(plain) == 4
