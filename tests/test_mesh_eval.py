"""CPU tests of the evaluator's mesh metrics (dis-pu_amd/mesh.py): OFF parsing, the face-tile layout, seed sampling, CGAL-file
I/O, argument validation, and the float64 oracle of tests/mesh_oracle.py on analytic cases.  No kernel runs here."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_oracle as MO  # noqa: E402

import dispu_amd  # noqa: E402,F401
from dispu_amd import mesh as M  # noqa: E402


@pytest.fixture(scope="module")
def pugan(golden_dir, tmp_path_factory):
    return MO.extract_pugan(golden_dir, str(tmp_path_factory.mktemp("pugan")))


@pytest.mark.parametrize("name,nv,nf", [("Icosahedron", 2562, 5120), ("fandisk", 2731, 5458)])
def test_load_off_fixtures(pugan, name, nv, nf):
    v, f = M.load_off(os.path.join(pugan, name + ".off"))
    assert v.shape == (nv, 3) and v.dtype == np.float32
    assert f.shape == (nf, 3) and f.dtype == np.int32
    assert f.min() == 0 and f.max() == nv - 1


def test_load_off_header_variants(tmp_path):
    body = "0 0 0\n1 0 0\n0 1 0\n0 0 1\n3 0 1 2\n3 0 2 3\n"
    p = tmp_path / "a.off"
    p.write_text("OFF 4 2 0\n" + body)
    v1, f1 = M.load_off(str(p))
    p.write_text("# comment\nOFF\n\n# counts next\n4 2 5\n" + body.replace("3 0 1 2\n", "3 0 1 2   # a face\n\n"))
    v2, f2 = M.load_off(str(p))
    assert np.array_equal(v1, v2) and np.array_equal(f1, f2)
    assert f1.tolist() == [[0, 1, 2], [0, 2, 3]]
    p.write_text("OFF\n4 2\n" + body)                        # no edge count
    assert np.array_equal(M.load_off(str(p))[1], f1)


@pytest.mark.parametrize("text,match", [
    ("PLY\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n", "OFF header"),
    ("OFF\n3\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n", "counts"),
    ("OFF\n3 1 0\n0 0 0\n1 0 0\n", "expected 3 vertex"),
    ("OFF\n3 1 0\n0 0 0\n1 0 x\n0 1 0\n3 0 1 2\n", "vertex line"),
    ("OFF\n4 1 0\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n", "only triangle"),
    ("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 7\n", "out of range"),
    ("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1\n", "fewer than 3"),
])
def test_load_off_rejects(tmp_path, text, match):
    p = tmp_path / "bad.off"
    p.write_text(text)
    with pytest.raises(ValueError, match=match):
        M.load_off(str(p))


def test_face_tiles_layout(pugan):
    v, f = M.load_off(os.path.join(pugan, "fandisk.off"))
    tris, order, box = M.face_tiles(v, f)
    F = f.shape[0]
    assert tris.shape == (F, 12) and box.shape == ((F + 63) // 64, 8)
    assert np.array_equal(np.sort(order), np.arange(F))
    assert np.array_equal(tris.reshape(F, 3, 4)[:, :, :3], v[f[order]]) and not tris.reshape(F, 3, 4)[:, :, 3].any()
    for t in range(box.shape[0]):
        pts = tris[64 * t:64 * t + 64].reshape(-1, 3, 4)[:, :, :3].reshape(-1, 3)
        assert np.array_equal(box[t, :3], pts.min(axis=0)) and np.array_equal(box[t, 4:7], pts.max(axis=0))
    # Morton order keeps tiles compact: far smaller boxes than tiles of faces in a random order
    ext = np.median((box[:, 4:7] - box[:, :3]).max(axis=1))
    shuffled = np.random.default_rng(0).permutation(F)
    tv = v[f[shuffled]][: (F // 64) * 64].reshape(-1, 64 * 3, 3)
    rext = np.median((tv.max(axis=1) - tv.min(axis=1)).max(axis=1))
    assert ext < 0.6 * rext


class _Areas(object):
    def __init__(self, areas):
        self.cum_areas = np.concatenate([[0.0], np.cumsum(areas / np.sum(areas))])


def test_find_surface_and_seeds():
    cum = np.array([0.0, 0.25, 0.75, 1.0])
    assert M.find_surface(cum, [0.0, 0.2499, 0.25, 0.9, 1.0]).tolist() == [0, 0, 1, 2, 0]   # u == 1 -> 0 as evaluation.cpp:123
    mesh = _Areas(np.array([1.0, 3.0, 0.0, 6.0]))
    fid, bary = M.sample_surface_seeds(mesh, count=20000, seed=3)
    assert fid.shape == (20000,) and bary.shape == (20000, 3)
    assert np.allclose(bary.sum(axis=1), 1.0) and bary.min() > 0.01 / 2.98
    frac = np.bincount(fid, minlength=4) / 20000.0
    assert frac[2] == 0 and abs(frac[0] - 0.1) < 0.01 and abs(frac[1] - 0.3) < 0.015 and abs(frac[3] - 0.6) < 0.015
    fid2, bary2 = M.sample_surface_seeds(mesh, count=20000, seed=3)
    assert np.array_equal(fid, fid2) and np.array_equal(bary, bary2)


def test_cgal_files_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    pts = rng.standard_normal((50, 3)).astype(np.float32)
    dist = rng.random(50).astype(np.float32)
    proj = rng.standard_normal((50, 3)).astype(np.float32)
    radii = np.array([0.1234567, 0.2], np.float32)
    rows = [sorted(rng.choice(50, size=k, replace=False).tolist()) for k in (0, 3, 7, 50, 1, 9)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    mem = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32)
    pred = str(tmp_path / "shape.xyz")
    M.write_cgal_files(pred, pts, dist, proj, radii, off, mem)
    p2m, rad, idx = M.cgal_paths(pred)
    assert os.path.basename(p2m) == "shape_point2mesh_distance.txt" and os.path.basename(idx) == "shape_disk_idx.txt"
    lines = open(idx).read().splitlines()
    assert len(lines) == 6 and lines[0] == "0:" and lines[1].startswith("3:")
    back = M.read_cgal_files(pred)
    assert np.array_equal(back["points"], pts) and np.array_equal(back["dist"], dist) and np.array_equal(back["proj"], proj)
    assert np.array_equal(back["radii"].astype(np.float32), radii)
    assert np.array_equal(back["offsets"], off) and np.array_equal(back["members"], mem)
    # the reference's own reader (evaluate.py:55-57): columns 4: of the distance file, radii by np.loadtxt
    assert np.array_equal(np.loadtxt(p2m).astype(np.float32)[:, 4:], proj)
    with open(idx, "a") as f:
        f.write("1:50 \n1:0 \n")                    # index past the 50 projected points
    with pytest.raises(ValueError, match="outside"):
        M.read_cgal_files(pred)


def test_shims_refuse_cpu_tensors():
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="must live on a ROCm device"):
        M.point_to_mesh(x, None)
    with pytest.raises(ValueError, match="must live on a ROCm device"):
        M.disk_members(x, x, [0.1])
    with pytest.raises(ValueError, match="must live on a ROCm device"):
        M.mean_std(torch.zeros(4))
    with pytest.raises(ValueError, match="must live on a ROCm device"):
        M.Mesh(np.zeros((3, 3)), np.array([[0, 1, 2]]), device="cpu")


# ---- the oracle on analytic cases ------------------------------------------------------------------------------------------
TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


@pytest.mark.parametrize("p,q", [
    ((0.2, 0.3, 1.0), (0.2, 0.3, 0.0)),          # face interior, above
    ((0.2, 0.3, -2.0), (0.2, 0.3, 0.0)),         # below
    ((-1.0, -1.0, 0.5), (0.0, 0.0, 0.0)),        # vertex a
    ((3.0, -0.5, 0.0), (1.0, 0.0, 0.0)),         # vertex b
    ((-0.1, 4.0, 0.0), (0.0, 1.0, 0.0)),         # vertex c
    ((0.5, -1.0, 0.0), (0.5, 0.0, 0.0)),         # edge ab
    ((-2.0, 0.25, 1.0), (0.0, 0.25, 0.0)),       # edge ca
    ((2.0, 2.0, 0.0), (0.5, 0.5, 0.0)),          # edge bc
    ((0.25, 0.25, 0.0), (0.25, 0.25, 0.0)),      # on the face
])
def test_oracle_closest_point(p, q):
    d2, Q = MO.closest_on_triangles(np.array([p]), TRI[None, 0], TRI[None, 1], TRI[None, 2])
    assert np.allclose(Q[0, 0], q, atol=1e-15)
    assert abs(math.sqrt(d2[0, 0]) - np.linalg.norm(np.subtract(p, q))) < 1e-15


def test_oracle_degenerate_triangles():
    line = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])      # collinear
    d2, Q = MO.closest_on_triangles(np.array([[1.5, 1.0, 0.0], [-1.0, 0.0, 0.0]]), line[None, 0], line[None, 1], line[None, 2])
    assert np.allclose(np.sqrt(d2[:, 0]), [1.0, 1.0]) and np.allclose(Q[:, 0], [[1.5, 0, 0], [0, 0, 0]])
    pt = np.array([[1.0, 2.0, 3.0]] * 3)                          # all three vertices coincide
    d2, Q = MO.closest_on_triangles(np.array([[1.0, 2.0, 5.0]]), pt[None, 0], pt[None, 1], pt[None, 2])
    assert np.isclose(np.sqrt(d2[0, 0]), 2.0) and np.allclose(Q[0, 0], [1, 2, 3])


def test_oracle_point_to_mesh_tie_and_gap():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    f = np.array([[1, 3, 2], [0, 1, 2]])                          # share the edge 1-2
    d, q, face, gap = MO.point_to_mesh(np.array([[0.5, 0.5, 1.0], [0.1, 0.1, 1.0]]), v, f)
    assert face.tolist() == [0, 1] and np.allclose(d, [1.0, 1.0])
    assert gap[0] == 0.0 and gap[1] > 0.1                         # on the shared edge: an exact tie -> the lower index


def test_oracle_analyze_uniform_by_hand():
    # five collinear points 0.1 apart -> every nearest other member is 0.1
    pts = np.array([[0.1 * k, 0, 0] for k in range(5)] + [[5.0, 5, 5]] * 5, np.float32)
    r = np.array([0.3, 0.05])
    disks = [[0, 1, 2, 3, 4], [0, 1], [5, 6, 7], []]               # seed 0: (r0, r1); seed 1: (r0, r1)
    pct = (0.2, 0.1)
    got = MO.analyze_uniform(disks, r, pts, pct)
    expect = 0.2 * 10
    coverage = (5 - expect) ** 2 / expect
    expect_d = math.sqrt(2 * (math.pi * 0.3 ** 2 / 5) / 1.732)
    nn = np.float64(np.float32(0.1) * 1)                          # float32 coordinates, float64 distances
    want0 = coverage * ((np.linalg.norm(pts[1] - pts[0].astype(np.float64)) - expect_d) ** 2 / expect_d)
    assert abs(nn - 0.1) < 1e-7
    assert np.isclose(got[0], want0, rtol=1e-6)                    # the 3-point disk of seed 1 is skipped (< 5)
    assert np.isnan(got[1])                                        # every r1 disk skipped -> NaN


# ---- the oracle helpers and inputs of tests/test_mesh_eval_ops_gpu.py ------------------------------------------------------------------
def test_uniform_terms_by_hand():
    # six points on a line, 0.25 apart (exact in float32), the last a copy of the first: nn = 0 for the pair, 0.25 for the rest
    pts = np.array([[0.25 * k, 0, 0] for k in range(5)] + [[0.0, 0, 0]] + [[9.0, 9, 9]] * 4, np.float32)
    disks = [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3], [6, 7, 8, 9], [4, 3, 2, 1, 0]]   # seed 0: (r0, r1); seed 1: (r0, r1)
    r, pct, N = np.array([0.5, 0.75]), np.array([0.01, 0.02]), 400
    kept, term, mean = MO.uniform_terms(disks, r, pts, pct, N)
    assert kept.tolist() == [1, 0, 0, 1] and term[1] == 0.0 and term[2] == 0.0
    ed0 = math.sqrt(2 * (math.pi * 0.25 / 6) / 1.732)
    want0 = (6 - 4.0) ** 2 / 4.0 * ((2 * (0 - ed0) ** 2 + 4 * (0.25 - ed0) ** 2) / ed0 / 6)
    ed3 = math.sqrt(2 * (math.pi * 0.5625 / 5) / 1.732)
    want3 = (5 - 8.0) ** 2 / 8.0 * ((0.25 - ed3) ** 2 / ed3)
    assert abs(term[0] - want0) <= 1e-15 * want0 and abs(term[3] - want3) <= 1e-15 * want3
    assert mean[0] == term[0] and mean[1] == term[3]                # one kept disk per radius
    _, _, none = MO.uniform_terms(disks[1:3], r, pts, pct, N)
    assert np.isnan(none).all()


def test_uniform_terms_against_analyze_uniform():
    rng = np.random.default_rng(12)
    pts = rng.random((600, 3)).astype(np.float32)
    pts[17] = pts[5]
    disks = [np.sort(rng.choice(600, c, replace=False)) for c in (300, 4, 5, 40, 0, 7, 257, 6, 64, 3)]   # S = 5, R = 2
    r, pct = np.array([0.4, 0.15]), np.array([0.3, 0.02])
    kept, term, mean = MO.uniform_terms(disks, r, pts, pct, 600)
    assert kept.tolist() == [int(len(d) >= 5) for d in disks]
    np.testing.assert_allclose(mean, MO.analyze_uniform(disks, r, pts, pct), rtol=1e-4)


def test_geodesic_disk_members_by_hand():
    r = np.array([0.1, 0.25], np.float32)
    r0 = float(r[0])                                              # float64(float32(0.1)) = 0.10000000149..., not 0.1
    off = np.array([0, 0, 4, 5])
    cand = np.array([7, 3, 9, 1, 2], np.int32)
    dist = np.array([r0, np.nextafter(r0, np.inf), np.inf, 0.0, 0.25])
    rows = MO.geodesic_disk_members(off, cand, dist, r)
    assert [x.tolist() for x in rows] == [[], [], [7, 1], [7, 3, 1], [], [2]]
    assert 0.1 < r0 and MO.geodesic_disk_members(off, cand, np.full(5, 0.1), r)[2].tolist() == [7, 3, 9, 1]


def test_geodesic_case_holds_its_special_distances():
    r = np.array([0.25, 0.1, 0.4], np.float32)
    off, cand, dist = MO.geodesic_case(MO.GEO_ROWS, r, seed=1)
    assert off.tolist() == [0, 0, 1, 64, 128, 193, 393] and cand.shape == dist.shape == (393,)
    r64 = r.astype(np.float64)
    for i in range(2, 6):
        row = dist[off[i]:off[i + 1]]
        assert row[0] == r64[i % 3] and row[1] > r64[i % 3] and np.float32(row[1]) == r[i % 3] and np.isinf(row[2]) and row[3] == 0.0
        assert np.all(np.diff(cand[off[i]:off[i + 1]]) > 0)
    assert dist[0] == r64[1]                                       # the row of one candidate: exactly on a radius


@pytest.mark.parametrize("case", [(1, 1, 1), (3, 63, 2), (6, 65, 3), (683, 65, 3)])
def test_disk_case_sits_on_the_radius(case):
    S, n, R = case
    seeds, points, radii = MO.disk_case(S, n, R)
    assert seeds.dtype == points.dtype == radii.dtype == np.float32 and radii[0] == 1e5
    r2 = MO.DISK_R * MO.DISK_R
    assert points[0, 0] * points[0, 0] == r2 and not seeds[0].any()
    rows = MO.disk_members_fp32(seeds, points, radii)
    assert all(np.array_equal(rows[i * R], np.arange(n)) for i in range(S))
    if n > 1 and R > 1:
        assert points[1, 0] * points[1, 0] > r2 and 0 in rows[1] and 1 not in rows[1]
    if S > 1 and R > 2:
        assert rows[1 * R + 2].tolist() == [n - 1]                 # radius 0: the point the seed copies, d2 = 0 <= 0


def test_uniformity_rows_layout():
    pts = MO.uniformity_points()
    assert pts.shape == (1100, 3) and np.array_equal(pts[0], pts[1099]) and len(np.unique(pts, axis=0)) == 1099
    for S in (1, 63, 65, 130):
        rows = MO.uniformity_rows(S)
        sizes = np.array([len(r) for r in rows]).reshape(S, 2)
        assert all(len(set(r.tolist())) == len(r) and r.min() >= 0 and r.max() < 1100 for r in rows if len(r))
        if S == 1:
            assert sizes.tolist() == [[1025, 5]]
            continue
        assert set(sizes.reshape(-1).tolist()) == set(MO.UNI_SIZES_KEPT + MO.UNI_SIZES_SKIPPED)
        assert (sizes[0::2, 0] >= 5).all() and (sizes[1::2, 0] < 5).all()                   # alternate along the seeds
        if S == 65:
            assert (sizes[:, 1] < 5).all()
        else:
            assert (sizes[1::2, 1] >= 5).all() and (sizes[0::2, 1] < 5).all()
        big = [r for r in rows if len(r) == 1025]
        paired = [r for r in big if r[0] == 0 and r[1024] == 1099]
        plain = [r for r in big if 0 not in r and 1099 not in r]
        assert len(paired) >= 1 and len(plain) >= 1 and len(paired) + len(plain) == len(big)


def test_mesh_builders():
    v, f = MO.icosphere_prefix(4, 4097)
    assert f.shape == (4097, 3) and v.dtype == np.float32 and f.max() < v.shape[0]
    v, f = MO.icosphere_prefix(2, None, 0.5, (37.5, -20.25, 11.0))
    assert f.shape == (320, 3) and np.allclose(np.linalg.norm(v - np.float32([37.5, -20.25, 11.0]), axis=1), 0.5, atol=1e-5)
    v, f = MO.sliver_rungs()
    tv = v[f].astype(np.float64)
    assert f.shape == (200, 3) and len(np.unique(f)) == 600
    assert np.allclose(np.linalg.norm(tv[:, 1] - tv[:, 0], axis=1), 1.0) and np.allclose(np.linalg.norm(tv[:, 2] - tv[:, 1], axis=1), 1e-4, rtol=1e-2)
    for extra, exact in ((MO.zero_area_faces(), True), (MO.near_collinear_faces(), False)):
        t = extra.astype(np.float64)
        area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
        assert (area == 0.0).all() if exact else (area.max() < 1e-8 and (area > 0).any())
        v2, f2 = MO.append_faces(v, f, extra)
        assert np.array_equal(v2[f2[200:]], extra) and np.array_equal(f2[:200], f)
    z = MO.zero_area_faces()
    same = [[bool(np.array_equal(t[a], t[b])) for a, b in ((0, 1), (1, 2), (0, 2))] for t in z]
    assert same == [[True, False, False], [False, True, False], [False, False, True], [True, True, True]] + [[False] * 3] * 3
    dv_, df = MO.duplicated(v, f)
    assert df.shape == (400, 3) and np.array_equal(df[:200], df[200:])


@pytest.mark.parametrize("name", MO.P2F_MESHES + (MO.P2F_DUP_BASE,))
def test_p2f_cases_leave_few_near_ties(name):
    """what tests/test_mesh_eval_ops_gpu.py asserts of its inputs, from the oracle alone: at most a tenth of a mesh's points lie within
    1e-6 x scale of a second face, and the meshes with appended faces have points that those faces decide."""
    case = MO.p2f_case(name)
    assert [len(s) for s in case["sets"]] == list(MO.P2F_POINT_COUNTS) and case["points"].shape == (333, 3)
    clear = case["gap"] > 1e-6 * case["scale"]
    assert 1.0 - clear.mean() <= 0.10
    assert case["scale"] >= 1.0 and (case["scale"] > 37 if name == "offset" else case["scale"] < 7)
    if case["favour"] is not None:
        assert (np.isin(case["face"], case["favour"]) & clear).sum() >= 40
        assert set(case["favour"].tolist()) <= set(case["face"][clear].tolist())   # every appended face decides a point
