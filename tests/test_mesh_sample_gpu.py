"""GPU tests of the mesh sampler (dis-pu_amd/mesh_sample.py, csrc/mesh_sample.hip, csrc/poisson_disk.hip, tools/make_dataset.py) against
the sequential numpy restatements of tests/mesh_sample_oracle.py: faces, keep flags, selected indices exact; points, radii bit for bit."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import mesh_oracle as MO  # noqa: E402
import mesh_sample_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
TOOL = os.path.join(ROOT, "tools", "make_dataset.py")
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ fixtures ---------
@pytest.fixture(scope="module")
def mesh_dir(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("pugan")
    MO.extract_pugan(golden_dir, str(d))
    for name in MO.PUGAN_FILES:
        if name.endswith(".xyz"):
            os.remove(os.path.join(str(d), name))
    return str(d)


def _host_mesh(name, mesh_dir):
    """(verts f32, faces i32) of the three test meshes"""
    from dispu_amd import mesh as M
    if name == "triangle":
        return np.array([[0.25, -1.0, 3.0], [2.0, 0.5, -1.0], [-0.75, 1.5, 0.125]], f32), np.array([[0, 1, 2]], np.int32)
    if name == "four":                                    # face 1: three collinear vertices, area exactly 0
        verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [1, 1, 0.5], [0, 3, 1], [3, 3, -1]], f32)
        return verts, np.array([[0, 1, 2], [1, 3, 4], [1, 5, 2], [2, 6, 7]], np.int32)
    return M.load_off(os.path.join(mesh_dir, name + ".off"))


_MESHES, _ORACLE_SAMPLES = {}, {}


def _mesh(name, mesh_dir, dev):
    from dispu_amd import mesh as M
    if name not in _MESHES:
        v, f = _host_mesh(name, mesh_dir)
        _MESHES[name] = M.Mesh(v, f, dev)
    return _MESHES[name]


def _oracle_samples(name, mesh_dir, dev, seed, count=4097):
    """the oracle's samples of a mesh, computed once per (mesh, seed) at the largest count (sample i does not depend on the count)"""
    key = (name, seed)
    if key not in _ORACLE_SAMPLES or _ORACLE_SAMPLES[key][0].shape[0] < count:
        m = _mesh(name, mesh_dir, dev)
        _ORACLE_SAMPLES[key] = SO.sample_surface(m.verts, m.faces, m.cum_areas, count, seed)
    return tuple(a[:count] for a in _ORACLE_SAMPLES[key])


def _diag(m):
    return float(np.linalg.norm(m.verts.max(axis=0).astype(np.float64) - m.verts.min(axis=0).astype(np.float64)))


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _own_face_distance(points, verts, faces, face):
    """float64 distance of every point to a point of ITS face (an upper bound of its distance to the face, hence to the mesh): the least
    of the distances to the three edges and, where the foot of the perpendicular falls inside the triangle, to the plane.

    "Every point lies on its face" within 1e-6 of the bounding-box diagonal is asserted on this.  The device point_to_mesh picks the
    nearest face in fp32 and reports the fp64 distance to the face it picked; on fandisk (slivers down to an area of 6.6e-9) it reads up
    to 6.0e-6 for samples whose float64 distance to the mesh is at most 3.2e-8 (tests/mesh_oracle.py), so its reading is asserted too,
    against the error its face choice can have (_p2m_reading_bound)."""
    p = np.asarray(points, np.float64)
    tv = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    a, b, c = tv[:, 0], tv[:, 1], tv[:, 2]
    best = np.full(p.shape[0], np.inf)
    for u, w in ((a, b), (b, c), (c, a)):
        best = np.minimum(best, np.sqrt(MO._segment(p, u, w)[0]))
    nrm = np.cross(b - a, c - a)
    nn = np.sum(nrm * nrm, axis=1)
    ok = nn > 0
    t = np.where(ok, np.sum((p - a) * nrm, axis=1) / np.where(ok, nn, 1.0), 0.0)
    foot = p - t[:, None] * nrm
    inside = ok.copy()
    for u, w in ((a, b), (b, c), (c, a)):
        inside &= np.sum(np.cross(w - u, foot - u) * nrm, axis=1) >= 0.0
    plane = np.abs(t) * np.sqrt(nn)
    return np.where(inside, np.minimum(best, plane), best)


def _p2m_reading_bound(points, verts, faces, face, own):
    """Per sample, the largest distance the DEVICE point_to_mesh may report for a point that lies `own` (float64) from its face T.

    point_to_mesh (csrc/mesh_eval.hip) takes the face W whose fp32 squared distance is smallest and reports the fp64 distance to W.
    The fp32 closest point q~ of any face is a convex combination of its corners (the region tests leave v, w >= 0, v + w <= 1), so it
    lies on that face up to rho = 8 u max|coordinate|, u = 2^-24; hence dist(p, W) <= |p - q~_W| + rho <= |p - q~_T| (1 + 4u) + rho
    <= (own + e_T)(1 + 4u) + rho, where e_T is how far the fp32 closest point of the sample's OWN face is from the true one.
    e_T: with L the longest edge and A the area of T, the dot products d1..d6 carry 3u L^2, the region numerators va, vb, vc (differences
    of products of two of them) 20u L^4, their sum den = 4 A^2 55u L^4, so v = vb / den and w are off by at most 70u L^4 / (4 A^2 - 55u L^4)
    and q~ = a + ab v + ac w by twice that times L; a region decided the other way by such an error moves q~ by no more.  With
    kappa = L^2 / (2 A) this is e_T <= 140 u L kappa^2 / (1 - 55 u kappa^2), and never more than the diameter L of T.
    On well-shaped faces (kappa ~ 1.2) that is a few 1e-7 at this scale; on slivers it degrades to L: the issue's bound of 1e-6 of the
    bounding-box diagonal (held exactly by the float64 own-face check) cannot be read through this instrument there -- fandisk reads
    6.0e-6 for a sample 3.2e-8 from the mesh."""
    u = 2.0 ** -24
    tv = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    a, b, c = tv[:, 0], tv[:, 1], tv[:, 2]
    L = np.maximum(np.maximum(np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1)), np.linalg.norm(a - c, axis=1))
    A = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        k2 = (L * L / (2.0 * A)) ** 2
        e = np.where(55.0 * u * k2 < 1.0, 140.0 * u * L * k2 / (1.0 - 55.0 * u * k2), np.inf)
    e = np.minimum(np.nan_to_num(e, nan=np.inf), L)
    rho = 8.0 * u * float(np.abs(np.asarray(verts, np.float64)).max())
    return (np.asarray(own, np.float64) + e) * (1.0 + 4.0 * u) + rho


def _check_on_mesh(name, pts, fc, mm):
    """every sample lies on its face: exactly (float64, the bound the check was given) and as the device point_to_mesh reads it (held to
    the error that function's fp32 face choice can have on the sample's face, _p2m_reading_bound)"""
    from dispu_amd import mesh as M
    p, face = pts.cpu().numpy().reshape(-1, 3), np.asarray(fc).reshape(-1)
    own = _own_face_distance(p, mm.verts, mm.faces, face)
    read = M.point_to_mesh(pts.reshape(-1, 3).contiguous(), mm)[0].cpu().numpy().astype(np.float64)
    bound = _p2m_reading_bound(p, mm.verts, mm.faces, face, own)
    k = int(np.argmax(read / bound))
    print("%s: largest float64 distance of a sample to its face %.3g (bound %.3g); device point_to_mesh reads at most %.3g, %d of %d above "
          "%.3g; tightest against its own bound: %.3g of %.3g" % (name, own.max(), 1e-6 * _diag(mm), read.max(), int((read > 1e-6 * _diag(mm)).sum()),
                                                                 read.shape[0], 1e-6 * _diag(mm), read[k], bound[k]))
    assert own.max() <= 1e-6 * _diag(mm)
    assert np.all(read <= bound), "device point_to_mesh reads %.3g where at most %.3g is explained" % (read[k], bound[k])


# ------------------------------------------------------------------------------------------------------------------ sample_surface ---
@pytest.mark.parametrize("name", ["triangle", "four", "fandisk"])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
def test_sample_surface_matches_oracle(name, count, mesh_dir, dev):
    from dispu_amd import mesh_sample as S
    m = _mesh(name, mesh_dir, dev)
    pts, face, bary = S.sample_surface(m, count, seed=7, return_bary=True)
    op, of, ob = _oracle_samples(name, mesh_dir, dev, 7, count)
    assert pts.shape == (count, 3) and face.shape == (count,)
    assert np.array_equal(face.cpu().numpy(), of)
    assert pts.cpu().numpy().tobytes() == op.tobytes()
    assert bary.cpu().numpy().tobytes() == ob.tobytes()
    if name == "four":
        assert m.areas[1] == 0.0 and not (face.cpu().numpy() == 1).any()
    p2, f2 = S.sample_surface(m, count, seed=7)
    assert p2.cpu().numpy().tobytes() == op.tobytes() and np.array_equal(f2.cpu().numpy(), of)


def test_sample_surface_prefix_seeds_and_surface(mesh_dir, dev):
    from dispu_amd import mesh as M
    from dispu_amd import mesh_sample as S
    m = _mesh("fandisk", mesh_dir, dev)
    big, fbig = S.sample_surface(m, 4097, seed=7)
    small, fsmall = S.sample_surface(m, 100, seed=7)
    assert np.array_equal(big.cpu().numpy()[:100], small.cpu().numpy()) and np.array_equal(fbig.cpu().numpy()[:100], fsmall.cpu().numpy())
    other, fother = S.sample_surface(m, 4097, seed=8)
    assert not np.array_equal(other.cpu().numpy(), big.cpu().numpy()) and not np.array_equal(fother.cpu().numpy(), fbig.cpu().numpy())
    op, of, _ = _oracle_samples("fandisk", mesh_dir, dev, 8, 300)
    assert other.cpu().numpy()[:300].tobytes() == op.tobytes()
    for name, (pts, fc) in (("fandisk", (big, fbig)), ("four", S.sample_surface(_mesh("four", mesh_dir, dev), 4097, seed=7)),
                            ("triangle", S.sample_surface(_mesh("triangle", mesh_dir, dev), 4097, seed=7))):
        _check_on_mesh(name, pts, fc.cpu().numpy(), _mesh(name, mesh_dir, dev))
    share = np.bincount(fbig.cpu().numpy(), minlength=m.num_faces)[:50].sum() / 4097.0          # area weighting, coarsely
    assert abs(share - m.cum_areas[50]) < 0.02
    with pytest.raises(ValueError):
        S.sample_surface(m, 0)


# ------------------------------------------------------------------------------------------------------------------ keep -------------
def _plane(rng, b, n):
    p = np.zeros((b, n, 3), f32)
    p[:, :, :2] = rng.random((b, n, 2), dtype=f32)
    return p


def _sphere(rng, b, n):
    v = rng.standard_normal((b, n, 3))
    return (v / np.linalg.norm(v, axis=2, keepdims=True)).astype(f32)


def _keep_cases():
    rng = np.random.default_rng(2024)
    lattice = np.zeros((2, 64, 3), f32)
    lattice[:, :, 0] = 0.25 * np.arange(64, dtype=f32)
    outlier = _plane(rng, 1, 2000)
    outlier[0, 777] = (1e3, -1e3, 1e3)
    mixed = np.concatenate([_plane(rng, 1, 1000), _sphere(rng, 1, 1000)])
    return {
        "one-point": (_plane(rng, 1, 1), [0.1]),
        "two-identical": (np.full((1, 2, 3), 0.375, f32), [0.1]),
        "plane-3x64": (_plane(rng, 3, 64), [0.1, 0.1, 0.1]),
        "sphere-2x65": (_sphere(rng, 2, 65), [0.3, 0.3]),
        "plane-sphere-2x1000": (mixed, [0.03, 0.1]),
        "sphere-1x4096": (_sphere(rng, 1, 4096), [0.05]),
        "plane-1x20000": (_plane(rng, 1, 20000), [0.01]),
        "identical-1x1000": (np.full((1, 1000, 3), -2.5, f32), [1e-3]),
        # d2 of lattice neighbours is 0.0625 == fl(0.25 * 0.25) exactly: nothing conflicts at r = 0.25 (strict <), neighbours do one ulp above
        "lattice-strict": (lattice, [0.25, np.nextafter(f32(0.25), f32(1.0))]),
        "radii-0-and-huge": (_plane(rng, 4, 500), [0.0, 0.05, 5.0, 0.02]),
        "negative-radius": (_sphere(rng, 2, 100), [-1.0, 0.2]),
        "outlier-grid-cap": (outlier, [0.03]),
    }


_KEEP = _keep_cases()


@pytest.mark.parametrize("case", sorted(_KEEP))
def test_poisson_disk_keep_matches_sequential_greedy(case, dev):
    import torch
    from dispu_amd import _lib
    from dispu_amd import mesh_sample as S
    pts, radii = _KEEP[case]
    b, n, _ = pts.shape
    radii = np.asarray(radii, f32)
    want = np.stack([SO.poisson_keep(pts[c], radii[c]) for c in range(b)])
    t = _dev(pts, dev)
    keep, count = S.poisson_disk_keep(t, _dev(radii, dev))
    k = keep.cpu().numpy()
    assert k.dtype == np.uint8 and k.shape == (b, n) and set(np.unique(k)) <= {0, 1}
    assert np.array_equal(k.astype(bool), want), "first difference at %s" % (np.argwhere(k.astype(bool) != want)[:1],)
    assert np.array_equal(count.cpu().numpy(), want.sum(axis=1).astype(np.int32))
    keep2, count2 = S.poisson_disk_keep(t, _dev(radii, dev))
    assert keep2.cpu().numpy().tobytes() == k.tobytes() and torch.equal(count, count2)
    # the C entry itself: a clean status word per cloud
    L = _lib.lib()
    nbytes = L.dispu_poisson_disk_scratch_bytes(b, n)
    assert nbytes == b * n * 16
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    status = torch.full((b,), 77, dtype=torch.int32, device=dev)
    k3, c3, r = torch.empty_like(keep), torch.empty_like(count), _dev(radii, dev)
    _lib.check(L.dispu_poisson_disk_keep(b, n, _lib.ptr(t), _lib.ptr(r), _lib.ptr(k3), _lib.ptr(c3), _lib.ptr(scratch), nbytes, _lib.ptr(status),
                                         _lib.stream_ptr(dev)), "dispu_poisson_disk_keep")
    assert not status.cpu().numpy().any() and torch.equal(k3, keep)
    if case == "identical-1x1000":
        assert k[0, 0] == 1 and k.sum() == 1
    if case == "two-identical":
        assert k.tolist() == [[1, 0]]
    if case == "lattice-strict":
        assert k[0].all() and np.array_equal(k[1], (np.arange(64) % 2 == 0).astype(np.uint8))
    if case == "radii-0-and-huge":
        assert k[0].all() and k[2].sum() == 1
    if b == 1:                                             # an [n,3] cloud and a Python radius
        k1, c1 = S.poisson_disk_keep(t[0], float(radii[0]))
        assert k1.shape == (n,) and torch.equal(k1, keep[0]) and int(c1.item()) == int(count[0].item())


def test_poisson_disk_argument_errors(dev):
    import torch
    from dispu_amd import _lib
    from dispu_amd import mesh_sample as S
    p = torch.zeros((1, 10, 3), device=dev)
    with pytest.raises(ValueError, match="cannot select 11 of 10"):
        S.poisson_disk_select(p, 11, 0.1)
    with pytest.raises(ValueError, match="must live on a ROCm device"):
        S.poisson_disk_keep(torch.zeros((1, 10, 3)), 0.1)
    with pytest.raises(ValueError, match="must live on a ROCm device"):
        S.poisson_disk_select(torch.zeros((10, 3)), 5, 0.1)
    with pytest.raises(TypeError):
        S.poisson_disk_keep(np.zeros((10, 3), f32), 0.1)
    big = torch.zeros((1, _lib.POISSON_MAX_N + 1, 3), device=dev)
    with pytest.raises(ValueError, match="DISPU_POISSON_MAX_N"):
        S.poisson_disk_keep(big, 0.1)
    with pytest.raises(ValueError, match="DISPU_POISSON_MAX_N"):
        S.poisson_disk_select(big, 5, 0.1)
    with pytest.raises(ValueError, match="one radius per cloud"):
        S.poisson_disk_keep(torch.zeros((2, 10, 3), device=dev), [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="in \\[1, 4096\\]"):
        S.sort_rows(torch.zeros((1, 4097), dtype=torch.int32, device=dev))
    # the C entries refuse what the shims refuse
    L = _lib.lib()
    assert L.dispu_poisson_disk_keep(1, _lib.POISSON_MAX_N + 1, None, None, None, None, None, 0, None, None) != 0
    assert L.dispu_poisson_disk_select(1, 10, 11, 12, None, None, None, None, None, None, 0, None, None) != 0
    assert L.dispu_sort_rows_i32(1, 4097, None, None) != 0
    assert L.dispu_poisson_disk_scratch_bytes(3, 1000) == 3 * 1000 * 16


def test_poisson_disk_keep_at_the_largest_cloud(dev):
    """n = DISPU_POISSON_MAX_N: the largest LDS request and the 16-bit cell offsets at their top"""
    from dispu_amd import _lib
    from dispu_amd import mesh_sample as S
    n = _lib.POISSON_MAX_N
    pts = _plane(np.random.default_rng(5), 1, n)
    want = SO.poisson_keep(pts[0], 0.006)
    keep, count = S.poisson_disk_keep(_dev(pts, dev), 0.006)
    assert np.array_equal(keep.cpu().numpy()[0].astype(bool), want) and int(count[0].item()) == int(want.sum())


# ------------------------------------------------------------------------------------------------------------------ select -----------
def _hex(area, m):
    return math.sqrt(2.0 * area / (math.sqrt(3.0) * m))


def _check_selection(pts, idx, r, count, m, want):
    widx, wr, wcount = want
    assert idx.dtype == np.int32 and np.array_equal(idx, widx)
    assert f32(r).tobytes() == f32(wr).tobytes() and int(count) == wcount
    assert count >= m and np.all(np.diff(idx) > 0)
    if m > 1 and r > 0:
        assert SO.min_pair_d2_f32(pts[idx]) >= f32(f32(r) * f32(r))           # every pair at distance >= r, in the kernel's own arithmetic


@pytest.mark.parametrize("n,m,steps", [(1024, 256, 12), (1024, 256, 1), (4096, 1024, 12)])
def test_poisson_disk_select_matches_oracle(n, m, steps, mesh_dir, dev):
    from dispu_amd import mesh_sample as S
    mesh = _mesh("fandisk", mesh_dir, dev)
    pts = _oracle_samples("fandisk", mesh_dir, dev, 7, n)[0]
    r_hi = f32(_hex(mesh.total_area, m))
    want = SO.poisson_select(pts, m, r_hi, steps)
    idx, r, count = S.poisson_disk_select(_dev(pts, dev), m, float(r_hi), steps)
    assert idx.shape == (m,)
    _check_selection(pts, idx.cpu().numpy(), float(r.item()), int(count.item()), m, want)
    if steps == 12:
        print("n %d m %d: r %.6g (r_hi %.6g), surplus %d" % (n, m, float(want[1]), float(r_hi), want[2] - m))
        assert want[2] - m <= math.ceil(0.02 * m)                              # the oracle alone meets the cap ...
        assert int(count.item()) - m <= math.ceil(0.02 * m)                    # ... and so does the kernel
    else:
        assert float(r.item()) in (0.0, float(f32(0.5) * r_hi))


def test_poisson_disk_select_batch_with_per_cloud_r_hi(mesh_dir, dev):
    from dispu_amd import mesh_sample as S
    n, m = 4096, 1024
    clouds, r_hi = [], []
    for name, seed, factor in (("fandisk", 7, 1.0), ("Icosahedron", 7, 1.25), ("fandisk", 8, 2.0), ("Icosahedron", 8, 1.0)):
        clouds.append(_oracle_samples(name, mesh_dir, dev, seed, n)[0])
        r_hi.append(f32(factor * _hex(_mesh(name, mesh_dir, dev).total_area, m)))
    pts = np.stack(clouds)
    idx, r, count = S.poisson_disk_select(_dev(pts, dev), m, _dev(np.asarray(r_hi, f32), dev), 12)
    idx2, r2, count2 = S.poisson_disk_select(_dev(pts, dev), m, _dev(np.asarray(r_hi, f32), dev), 12)
    assert idx.cpu().numpy().tobytes() == idx2.cpu().numpy().tobytes() and r.cpu().numpy().tobytes() == r2.cpu().numpy().tobytes()
    assert idx.shape == (4, m) and r.shape == (4,) and count.shape == (4,)
    for c in range(4):
        want = SO.poisson_select(pts[c], m, r_hi[c], 12)
        _check_selection(pts[c], idx[c].cpu().numpy(), float(r[c].item()), int(count[c].item()), m, want)
        print("cloud %d: r %.6g (r_hi %.6g), surplus %d" % (c, float(want[1]), float(r_hi[c]), want[2] - m))
        assert want[2] - m <= math.ceil(0.02 * m) and int(count[c].item()) - m <= math.ceil(0.02 * m)


def test_poisson_disk_select_all_points_and_odd_r_hi(mesh_dir, dev):
    from dispu_amd import mesh_sample as S
    pts = _oracle_samples("Icosahedron", mesh_dir, dev, 7, 300)[0]
    for m, r_hi, steps in ((300, 0.5, 12), (300, 0.0, 12), (17, -1.0, 3), (1, 100.0, 12), (300, 0.5, 0)):
        want = SO.poisson_select(pts, m, f32(r_hi), steps)
        idx, r, count = S.poisson_disk_select(_dev(pts, dev), m, r_hi, steps)
        _check_selection(pts, idx.cpu().numpy(), float(r.item()), int(count.item()), m, want)
        if m == 300:
            assert np.array_equal(idx.cpu().numpy(), np.arange(300)) and int(count.item()) == 300
    assert int(S.poisson_disk_select(_dev(pts, dev), 1, 100.0)[0].item()) == 0


# ------------------------------------------------------------------------------------------------------------------ sort rows --------
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 1000, 4096])
@pytest.mark.parametrize("b", [1, 5])
def test_sort_rows_matches_numpy(b, k, dev):
    from dispu_amd import mesh_sample as S
    rng = np.random.default_rng(100 * b + k)
    a = rng.integers(-2 ** 31, 2 ** 31, (b, k), dtype=np.int64).astype(np.int32)
    a[0, : k // 3] = a[0, k // 3: 2 * (k // 3)]                                 # repeated values
    if k > 2:
        a[-1, 0], a[-1, 1] = 2 ** 31 - 1, -2 ** 31
    t = _dev(a, dev)
    out = S.sort_rows(t)
    assert out is t and np.array_equal(t.cpu().numpy(), np.sort(a, axis=1))
    perm = np.stack([rng.permutation(81920)[:k] for _ in range(b)]).astype(np.int32)    # what make_patches sorts: distinct indices
    assert np.array_equal(S.sort_rows(_dev(perm, dev)).cpu().numpy(), np.sort(perm, axis=1))


# ------------------------------------------------------------------------------------------------------------------ make_patches -----
@pytest.fixture(scope="module")
def fandisk_patches(mesh_dir, dev):
    from dispu_amd import mesh_sample as S
    mesh = _mesh("fandisk", mesh_dir, dev)
    inp, gt, det = S.make_patches(mesh, 8, oversample=4, seed=3, return_details=True)
    return mesh, inp, gt, {k: v.cpu().numpy() for k, v in det.items()}


def test_make_patches_shapes_and_oracle_pipeline(fandisk_patches, dev):
    from dispu_amd import mesh_sample as S
    from dispu_amd.tf_sampling import farthest_point_sample
    from dispu_amd.upsample import knn_patch
    mesh, inp, gt, det = fandisk_patches
    k, D = 4096, 81920
    assert inp.shape == (8, 256, 3) and gt.shape == (8, 1024, 3)
    dense, regions = det["dense"], det["regions"]
    assert dense.shape == (D, 3) and regions.shape == (8, k) and det["seeds"].shape == (8,)
    # the dense samples are the sampler's, the seeds the exact FPS's, the regions the k-NN rows in ascending order
    d_dev = _dev(dense, dev)
    assert S.sample_surface(mesh, D, seed=3)[0].cpu().numpy().tobytes() == dense.tobytes()
    assert dense[:2000].tobytes() == SO.sample_surface(mesh.verts, mesh.faces, mesh.cum_areas, 2000, 3)[0].tobytes()
    seeds = farthest_point_sample(8, d_dev.reshape(1, D, 3))
    assert np.array_equal(seeds.cpu().numpy()[0], det["seeds"])
    knn = knn_patch(d_dev.reshape(1, D, 3), d_dev[seeds[0].long()].reshape(1, 8, 3), k)[0].cpu().numpy()
    assert np.array_equal(np.sort(knn, axis=1), regions) and np.all(np.diff(regions, axis=1) > 0)
    # the oracle's selection over the same regions
    area = mesh.total_area * k / D
    gi, gg = inp.cpu().numpy(), gt.cpu().numpy()
    for name, num, got in (("in", 256, gi), ("gt", 1024, gg)):
        r_hi = f32(_hex(area, num))
        for p in range(8):
            cand = dense[regions[p]]
            widx, wr, wcount = SO.poisson_select(cand, num, r_hi, 12)
            assert np.array_equal(det["idx_" + name][p], widx)
            assert f32(det["r_" + name][p]).tobytes() == f32(wr).tobytes() and int(det["count_" + name][p]) == wcount
            assert got[p].tobytes() == cand[widx].tobytes()
            cv = SO.nn_cv(got[p])
            print("patch %d %s: r %.6g (r_hi %.6g), surplus %d, nearest-neighbour CV %.3f" % (p, name, float(wr), float(r_hi), wcount - num, cv))
            assert SO.min_pair_d2_f32(got[p]) >= f32(f32(wr) * f32(wr))
            assert cv <= 0.25


def test_make_patches_on_the_mesh_and_reproducible(fandisk_patches, dev):
    from dispu_amd import mesh as M
    from dispu_amd import mesh_sample as S
    mesh, inp, gt, det = fandisk_patches
    dense_face = S.sample_surface(mesh, 81920, seed=3)[1].cpu().numpy()          # the dense samples again (bit-identical, tested above)
    for t, name in ((inp, "in"), (gt, "gt")):
        src = np.take_along_axis(det["regions"], det["idx_" + name].astype(np.int64), axis=1)      # [8, num] dense sample of every point
        assert t.cpu().numpy().tobytes() == det["dense"][src].tobytes()
        _check_on_mesh("patches " + name, t, dense_face[src], mesh)
    inp2, gt2 = S.make_patches(mesh, 8, oversample=4, seed=3)
    assert inp2.cpu().numpy().tobytes() == inp.cpu().numpy().tobytes() and gt2.cpu().numpy().tobytes() == gt.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="at most 4096"):
        S.make_patches(mesh, 8, oversample=5)


def test_poisson_disk_cloud(mesh_dir, dev):
    from dispu_amd import mesh as M
    from dispu_amd import mesh_sample as S
    mesh = _mesh("Icosahedron", mesh_dir, dev)
    pts, r = S.poisson_disk_cloud(mesh, 512, oversample=4, seed=7)
    cand = _oracle_samples("Icosahedron", mesh_dir, dev, 7, 2048)[0]
    widx, wr, _ = SO.poisson_select(cand, 512, f32(S.hex_radius(mesh.total_area, 512)), 12)
    assert pts.shape == (512, 3) and pts.cpu().numpy().tobytes() == cand[widx].tobytes() and f32(r).tobytes() == f32(wr).tobytes()
    _check_on_mesh("Icosahedron cloud", pts, _oracle_samples("Icosahedron", mesh_dir, dev, 7, 2048)[1][widx], mesh)
    assert SO.nn_cv(pts.cpu().numpy()) <= 0.25
    assert abs(S.hex_radius(3.0, 100) - math.sqrt(6.0 / (math.sqrt(3.0) * 100))) < 1e-15


# ------------------------------------------------------------------------------------------------------------------ end to end -------
def test_tool_closes_the_loop(mesh_dir, tmp_path, dev):
    """meshes -> patches.h5 -> load_patches -> DeviceFetcher batch; meshes -> 2048 / 8192 clouds -> evaluate_pair"""
    from dispu_amd import dataset, evaluate
    from dispu_amd import mesh as M
    out = str(tmp_path / "data" / "PUGAN_poisson_256_poisson_1024.h5")
    r = subprocess.run([sys.executable, TOOL, "patches", "--mesh_dir", mesh_dir, "--out", out, "--patches_per_mesh", "4"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    names = open(out[:-3] + "_names.txt").read().split()
    assert names == ["Icosahedron"] * 4 + ["fandisk"] * 4
    inp, gt = dataset.load_patches(out, 256, 1024, random=False)
    assert inp.shape == (8, 256, 3) and gt.shape == (8, 1024, 3) and inp.dtype == np.float32
    fetcher = dataset.DeviceFetcher(*dataset.load_patches(out, 256, 1024, random=True), batch_size=4, device=dev, seed=1)
    bi, bg, br = fetcher.next_batch()
    assert bi.shape == (4, 256, 3) and bg.shape == (4, 1024, 3) and br.shape == (4,)
    assert all(bool(np.isfinite(t.cpu().numpy()).all()) for t in (bi, bg, br))
    for num in (2048, 8192):
        r = subprocess.run([sys.executable, TOOL, "clouds", "--mesh_dir", mesh_dir, "--out_dir", str(tmp_path / ("c%d" % num)), "--num", str(num)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode(errors="replace")
    lo = np.loadtxt(str(tmp_path / "c2048" / "fandisk.xyz"), dtype=np.float32)
    hi = np.loadtxt(str(tmp_path / "c8192" / "fandisk.xyz"), dtype=np.float32)
    assert lo.shape == (2048, 3) and hi.shape == (8192, 3) and sorted(os.listdir(str(tmp_path / "c2048"))) == ["Icosahedron.xyz", "fandisk.xyz"]
    res = evaluate.evaluate_pair(lo, hi, mesh=_mesh("fandisk", mesh_dir, dev))
    assert np.isfinite(res["CD"]) and np.isfinite(res["hausdorff"]) and res["CD"] > 0
    # the cloud lies on the mesh: fp32 rounding of the point as above, plus half a unit of the text format's sixth decimal per coordinate
    assert res["p2f avg"] <= 1e-6 * _diag(_mesh("fandisk", mesh_dir, dev)) + math.sqrt(3.0) * 0.5e-6
