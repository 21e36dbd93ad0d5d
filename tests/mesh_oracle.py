"""Float64 oracle of the evaluator's mesh metrics, for tests only (dis-pu_amd/mesh.py, csrc/mesh_eval.hip).

Written independently of the kernels: the closest point on a triangle here is the projection onto the supporting plane when it
falls inside the triangle (face region), otherwise the nearest point of the three edges as clamped segments (edge and vertex
regions); a triangle without area is its three edges.  The kernel walks Ericson's Voronoi-region tests instead.

  point_to_mesh      P2F with the best and second-best face per point (a near-tie indicator for the tolerances)
  disk_members_fp32  the membership test restated in float32: d2 = (dx*dx + dy*dy) + dz*dz <= fl32(r*r)
  analyze_uniform    evaluate.py:53-101 restated line by line, sklearn's 2-NN as the nearest other member in float64
  extract_pugan      the PU-GAN test meshes and network outputs of tests/golden/pugan_test_meshes.npz, as files
  uniform_terms      dispu_disk_uniformity's formula per disk as include/dispu_hip.h states it: (kept, term) and the per-radius mean
  geodesic_disk_members  dist[c] <= float64(float32 r_j) over hand-made candidate rows
  p2f_case, disk_case, geodesic_case, uniformity_rows  the meshes, points and rows of tests/test_mesh_eval_ops_gpu.py, built from
                     icosphere_prefix, sliver_rungs, zero_area_faces, near_collinear_faces, append_faces, duplicated, mesh_points
"""
import math
import os

import numpy as np


PUGAN_FILES = ("Icosahedron.off", "fandisk.off", "Icosahedron_X4.xyz", "fandisk_X4.xyz")


def extract_pugan(golden_dir, out_dir):
    """tests/golden/pugan_test_meshes.npz keeps four files of the reference's data/test byte for byte, as uint8 arrays under
    their names with '.' -> '_': the test meshes Icosahedron.off (2562 V / 5120 F) and fandisk.off (2731 V / 5458 F) and the
    network's 8192-point outputs output/{Icosahedron,fandisk}_X4.xyz.  Writes them into out_dir and returns out_dir."""
    z = np.load(os.path.join(golden_dir, "pugan_test_meshes.npz"))
    for name in PUGAN_FILES:
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(z[name.replace(".", "_")].tobytes())
    return out_dir


def _segment(P, A, B):
    """closest points of segments A-B [1,F,3] to points P [c,1,3] -> (d2 [c,F], Q [c,F,3])"""
    E = B - A
    ee = np.sum(E * E, axis=-1)
    t = np.where(ee > 0, np.sum((P - A) * E, axis=-1) / np.where(ee > 0, ee, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    Q = A + t[..., None] * E
    return np.sum((P - Q) ** 2, axis=-1), Q


def closest_on_triangles(P, A, B, C):
    """P [c,3] against triangles A, B, C [F,3] (float64) -> (d2 [c,F], Q [c,F,3])."""
    P = np.asarray(P, np.float64)[:, None, :]
    A, B, C = (np.asarray(X, np.float64)[None] for X in (A, B, C))
    N = np.cross(B - A, C - A)
    nn = np.sum(N * N, axis=-1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    t = np.sum((P - A) * N, axis=-1) / nn1
    Qf = P - t[..., None] * N
    u = np.sum(np.cross(C - B, Qf - B) * N, axis=-1) / nn1
    v = np.sum(np.cross(A - C, Qf - C) * N, axis=-1) / nn1
    w = 1.0 - u - v
    inside = ok & (u >= 0) & (v >= 0) & (w >= 0)
    best = np.where(inside, np.sum((P - Qf) ** 2, axis=-1), np.inf)
    Q = np.where(inside[..., None], Qf, 0.0)
    for X, Y in ((A, B), (B, C), (C, A)):
        d2, Qs = _segment(P, X, Y)
        take = d2 < best
        best = np.where(take, d2, best)
        Q = np.where(take[..., None], Qs, Q)
    return best, Q


def point_to_mesh(points, verts, faces, chunk=256):
    """-> dist [n] f64, proj [n,3] f64, face [n] (lowest index among exact ties), gap [n] = second-best face distance - best.

    Exact, with a cull that cannot drop the best two faces: a face is evaluated only if its bounding-sphere lower bound
    |p - centroid| - radius is <= U2, the second smallest over faces of the distance to the face's nearest vertex (an upper
    bound of the second-best face distance)."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    V = np.asarray(verts, np.float64)
    Fc = np.asarray(faces, np.int64)
    A, B, C = V[Fc[:, 0]], V[Fc[:, 1]], V[Fc[:, 2]]
    cen = (A + B + C) / 3.0
    rad = np.sqrt(np.max([np.sum((X - cen) ** 2, axis=1) for X in (A, B, C)], axis=0)) * (1 + 1e-12) + 1e-15
    n, F = pts.shape[0], Fc.shape[0]
    dist, gap = np.empty(n), np.full(n, np.inf)
    proj, face = np.empty((n, 3)), np.empty(n, np.int64)
    for s in range(0, n, chunk):
        P = pts[s:s + chunk]
        lb = np.sqrt(np.sum((P[:, None, :] - cen[None]) ** 2, axis=-1)) - rad[None]
        vd = np.sqrt(np.sum((P[:, None, :] - V[None]) ** 2, axis=-1))
        ub = vd[:, Fc].min(axis=2)
        u2 = np.partition(ub, 1, axis=1)[:, 1] if F > 1 else ub[:, 0]
        for i in range(P.shape[0]):
            idx = np.nonzero(lb[i] <= u2[i] * (1 + 1e-12) + 1e-15)[0]
            d2, Q = closest_on_triangles(P[i:i + 1], A[idx], B[idx], C[idx])
            d = np.sqrt(d2[0])
            k = int(np.argmin(d))                      # first minimum in ascending face order = lowest face index
            dist[s + i], proj[s + i], face[s + i] = d[k], Q[0, k], idx[k]
            if idx.shape[0] > 1:
                d[k] = np.inf
                gap[s + i] = d.min() - dist[s + i]
    return dist, proj, face, gap


def disk_members_fp32(seeds, points, radii):
    """float32 restatement of the membership test -> list over (i, j), seed-major, of ascending index arrays."""
    s = np.asarray(seeds, np.float32).reshape(-1, 3)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    r = np.asarray(radii, np.float32).reshape(-1)
    out = []
    for i in range(s.shape[0]):
        dx, dy, dz = p[:, 0] - s[i, 0], p[:, 1] - s[i, 1], p[:, 2] - s[i, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        for j in range(r.shape[0]):
            out.append(np.nonzero(d2 <= r[j] * r[j])[0])
    return out


def geodesic_disk_members(cand_off, cand, dist, radii):
    """Geodesic membership from given distances (include/dispu_hip.h: dispu_geodesic_disk_count): candidate c of seed i is in disk
    (i, j) iff dist[c] <= float64(float32 r_j) -> list over (i, j), seed-major, of the members cand[c] in candidate order."""
    off = np.asarray(cand_off, np.int64).reshape(-1)
    cand = np.asarray(cand, np.int32).reshape(-1)
    dist = np.asarray(dist, np.float64).reshape(-1)
    r = np.asarray(radii, np.float32).reshape(-1).astype(np.float64)
    out = []
    for i in range(off.shape[0] - 1):
        b, e = int(off[i]), int(off[i + 1])
        for j in range(r.shape[0]):
            out.append(cand[b:e][dist[b:e] <= r[j]])
    return out


def uniform_terms(disks, radius, points, pct, N):
    """The header's formula of dispu_disk_uniformity per disk: disks = list of index rows, seed-major with R = len(radius) per seed,
    points [n,3] float32, expect = pct[j] * N.  -> (kept [S*R] int32, term [S*R] f64, mean [R] f64).
    A row of c < 5 members is skipped (kept 0, term 0).  Otherwise nn_a = sqrt of the smallest d2 to another ROW POSITION (a repeated
    index or a coincident point is another member at distance 0), d2 = (dx*dx + dy*dy) + dz*dz in float32 of float32 differences -- a
    minimum of float32 values, so exact in any order -- and everything after it float64:
    term = (c - expect)^2 / expect * mean_a((nn_a - expect_d)^2 / expect_d), expect_d = sqrt(2 (pi r^2 / c) / 1.732), the sums by
    math.fsum (correctly rounded).  mean[j] = the mean of the kept terms of radius j, NaN without any."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    radius = np.asarray(radius, np.float64).reshape(-1)
    pct = np.asarray(pct, np.float64).reshape(-1)
    R = radius.shape[0]
    assert len(disks) % R == 0 and pct.shape[0] == R
    kept, term = np.zeros(len(disks), np.int32), np.zeros(len(disks), np.float64)
    for k, row in enumerate(disks):
        c, j = len(row), k % R
        if c < 5:
            continue
        m = pts[np.asarray(row, np.int64)]
        dx, dy, dz = (m[None, :, a] - m[:, None, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        np.fill_diagonal(d2, np.inf)
        nn = np.sqrt(d2.min(axis=1).astype(np.float64))
        expect = pct[j] * float(N)
        coverage = (c - expect) * (c - expect) / expect
        expect_d = math.sqrt(2.0 * (math.pi * radius[j] * radius[j] / c) / 1.732)
        e = nn - expect_d
        term[k] = coverage * (math.fsum(e * e / expect_d) / c)
        kept[k] = 1
    mean = np.full(R, np.nan)
    for j in range(R):
        sel = np.nonzero(kept[j::R])[0] * R + j
        if sel.size:
            mean[j] = math.fsum(term[sel]) / sel.size
    return kept, term, mean


# ---- meshes and points of the kernel-level P2F tests (tests/test_mesh_eval_ops_gpu.py) -----------------------------------------
def icosphere_prefix(level, F=None, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """synth.icosphere(level, radius) moved to `centre` (float32 sum) and cut to its first F faces (all when None); the vertices the
    cut no longer uses stay in the vertex list."""
    from dispu_amd import synth
    v, f = synth.icosphere(level, radius)
    v = (v + np.asarray(centre, np.float32)[None]).astype(np.float32)
    return v, (f if F is None else f[:F]).copy()


def sliver_rungs(count=200, length=1.0, width=1e-4):
    """A strip of `count` slivers: right triangles of the given length (along x) and width (along y) laid side by side like the rungs
    of a ladder, 1 / count apart in y with a slow wave in z, sharing no vertex.  Slivers that shared their long edges would put every
    point further than a width from the strip within 1e-6 of two faces at once, and no face could be asserted."""
    k = np.arange(count, dtype=np.float64)
    y, z = k / count, 0.02 * np.sin(k * 0.37)
    a = np.stack([np.zeros(count), y, z], 1)
    b = np.stack([np.full(count, length), y, z], 1)
    c = np.stack([np.full(count, length), y + width, z], 1)
    v = np.stack([a, b, c], 1).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * count, dtype=np.int32).reshape(count, 3)


def append_faces(verts, faces, tri_verts):
    """the mesh plus one face per [3,3] entry of tri_verts (their vertices appended, unshared)."""
    t = np.asarray(tri_verts, np.float32).reshape(-1, 3)
    f = (np.arange(t.shape[0], dtype=np.int32) + verts.shape[0]).reshape(-1, 3)
    return np.concatenate([verts, t]).astype(np.float32), np.concatenate([faces, f]).astype(np.int32)


def zero_area_faces(z=0.5):
    """[7,3,3] float32 faces without area, 0.25 or more apart on the plane z: two vertices equal (each of the three pairs), all three
    equal, and three distinct, exactly collinear vertices along (4, 2, 1) / 32 with the middle one listed first, second and last."""
    out = []
    for i, same in enumerate(((0, 1), (1, 2), (0, 2))):
        t = np.array([[0.125 + 0.25 * i, 0.125, z]] * 3)
        t[[k for k in range(3) if k not in same][0]] += (0.125, 0.0625, 0.03125)
        out.append(t)
    out.append(np.array([[0.875, 0.125, z]] * 3))
    step = np.array([0.125, 0.0625, 0.03125])
    for i, order in enumerate(((1, 0, 2), (0, 1, 2), (0, 2, 1))):                 # parameters 0, 1, 3 along the line
        a = np.array([0.125 + 0.25 * i, 0.625, z])
        line = np.stack([a, a + step, a + 3.0 * step])
        out.append(line[list(order)])
    t = np.asarray(out, np.float32)
    assert np.array_equal(t.astype(np.float64), np.asarray(out, np.float64))      # every coordinate is a float32 as written
    return t


def near_collinear_faces(count=12, z=0.5, seed=0):
    """[count,3,3] float32: a + t d for three t of a random line each, exactly collinear in float64 and then rounded to float32 --
    faces whose area is what the rounding left (about 1e-8), on a 4 x 3 grid over the plane z, in every vertex order."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        a = np.array([0.125 + 0.25 * (i % 4), 0.2 + 0.3 * (i // 4), z]) + rng.uniform(-0.01, 0.01, 3)
        d = rng.standard_normal(3)
        d *= 0.03 / np.linalg.norm(d)
        t = np.array([0.0, rng.uniform(0.2, 0.8), 1.0]) * 2.0
        out.append((a[None] + t[:, None] * d[None])[rng.permutation(3)])
    return np.asarray(out, np.float64).astype(np.float32)


def duplicated(verts, faces):
    """the mesh with its face list appended to itself: faces F0 .. 2 F0 - 1 repeat faces 0 .. F0 - 1 vertex for vertex, so every
    point is at exactly the same float32 distance from face i and face i + F0."""
    return verts, np.concatenate([faces, faces]).astype(np.int32)


def mesh_points(verts, faces, n, seed, favour=None):
    """n test points [n,3] float32 for a mesh, a fixed mix by position.  From n = 16 on: 2.5 % mesh vertices, 2.5 % edge midpoints,
    2.5 % points 3 mesh sizes from the centre and, last, the centre of the bounding box -- on a closed, convex mesh all four kinds
    are ties or near-ties between the faces around a vertex or an edge, so together they stay below the tenth of the points that the
    face comparison may leave out.  The rest, and every point of a smaller set, in equal parts: face interiors, points above and
    points below a face by 1e-3 .. 5e-2 of the mesh size along its normal (along z for a face without area).
    `favour`: face indices that a quarter of the points are drawn from (the rest from every face)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64)
    fc = np.asarray(faces, np.int64)
    tv = v[fc]
    used = tv.reshape(-1, 3)
    lo, hi = used.min(axis=0), used.max(axis=0)
    size, centre = float((hi - lo).max()), 0.5 * (lo + hi)
    fid = rng.integers(0, fc.shape[0], n)
    if favour is not None:
        pick = rng.random(n) < 0.25
        fid = np.where(pick, np.asarray(favour, np.int64)[rng.integers(0, len(favour), n)], fid)
    nrm = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0])[None])
    b = rng.random((n, 3)) + 0.05
    b /= b.sum(axis=1, keepdims=True)
    on = np.einsum("nk,nkc->nc", b, tv[fid])
    h = rng.uniform(1e-3, 5e-2, n)[:, None] * size * nrm[fid]
    g = rng.standard_normal((n, 3))
    far = centre[None] + 3.0 * size * g / np.linalg.norm(g, axis=1, keepdims=True)
    nv = int(round(0.025 * n)) if n >= 16 else 0
    kind = np.concatenate([np.repeat([0, 1, 5], nv), 2 + np.arange(n - 3 * nv) % 3])
    pts = on.copy()                                                              # kind 2: face interior
    pts[kind == 0] = tv[fid, 0][kind == 0]
    pts[kind == 1] = 0.5 * (tv[fid, 0] + tv[fid, 1])[kind == 1]
    pts[kind == 3] = (on + h)[kind == 3]
    pts[kind == 4] = (on - h)[kind == 4]
    pts[kind == 5] = far[kind == 5]
    if nv:
        pts[n - 1] = centre
    return pts.astype(np.float32)


P2F_POINT_COUNTS = (1, 3, 4, 5, 63, 257)


def _p2f_mesh(name):
    if name.startswith("ico2_"):
        return icosphere_prefix(2, int(name[5:])) + (None,)
    if name.startswith("ico4_"):
        return icosphere_prefix(4, int(name[5:])) + (None,)
    if name == "offset":
        return icosphere_prefix(2, None, 0.5, (37.5, -20.25, 11.0)) + (None,)
    if name == "rungs":
        return sliver_rungs() + (None,)
    if name in ("rungs_zero", "rungs_collinear"):
        v, f = sliver_rungs()
        extra = zero_area_faces() if name == "rungs_zero" else near_collinear_faces()
        v2, f2 = append_faces(v, f, extra)
        return v2, f2, np.arange(f.shape[0], f2.shape[0])
    raise KeyError(name)


P2F_MESHES = ("ico2_1", "ico2_20", "ico2_63", "ico2_64", "ico2_65", "ico4_4096", "ico4_4097", "ico4_5120", "offset", "rungs",
              "rungs_zero", "rungs_collinear")
P2F_DUP_BASE = "ico2_320"                 # the mesh the two duplicated cases repeat
_P2F_CACHE = {}


def p2f_case(name):
    """-> dict(verts, faces, favour, sets = one point array per P2F_POINT_COUNTS, points = their concatenation, scale =
    max(1, largest |coordinate| of mesh and points), and the oracle's dist / proj / face / gap over `points`), computed once."""
    if name not in _P2F_CACHE:
        v, f, favour = _p2f_mesh(name)
        seed0 = sum(ord(ch) for ch in name)
        sets = [mesh_points(v, f, n, seed=1000 * seed0 + n, favour=favour) for n in P2F_POINT_COUNTS]
        pts = np.concatenate(sets)
        used = v[np.asarray(f, np.int64)].reshape(-1, 3)
        scale = max(1.0, float(np.abs(used).max()), float(np.abs(pts).max()))
        d, q, face, gap = point_to_mesh(pts, v, f)
        _P2F_CACHE[name] = {"verts": v, "faces": f, "favour": favour, "sets": sets, "points": pts, "scale": scale, "dist": d,
                            "proj": q, "face": face, "gap": gap}
    return _P2F_CACHE[name]


# ---- inputs of the kernel-level disk tests -------------------------------------------------------------------------------------
DISK_R = np.float32(0.3)                                   # the radius with a point exactly on it
DISK_RADII = np.array([1e5, 0.3, 0.0, 0.8, 1.3], np.float32)   # the first R of these per call: every point; the edge; the seed only


def disk_case(S, n, R, seed=0):
    """-> seeds [S,3], points [n,3], radii [R] float32.  Seed 0 is the origin, point 0 is (r, 0, 0) with r = DISK_R, so that
    d2 == fl32(r * r) exactly, point 1 (n > 1) is one float32 further out, whose d2 is the next value or more; seed 1 (S > 1) is a
    copy of the last point (d2 = 0 <= 0 at radius 0).  Everything else is uniform in [-1, 1]^3.  1e5 is beyond any guard value read
    as a coordinate (|-12345| sqrt 3 < 2.2e4), so a lane that read past the points would count."""
    rng = np.random.default_rng(seed + 7 * S + 13 * n + R)
    seeds = rng.uniform(-1, 1, (S, 3)).astype(np.float32)
    points = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    seeds[0] = 0.0
    points[0] = (DISK_R, 0.0, 0.0)
    if n > 1:
        points[1] = (np.nextafter(DISK_R, np.float32(1.0)), 0.0, 0.0)
    if S > 1:
        seeds[1] = points[n - 1]
    return seeds, points, DISK_RADII[:R].copy()


GEO_ROWS = (0, 1, 63, 64, 65, 200)


def geodesic_case(lengths, radii, seed=0, universe=1000):
    """Hand-made candidates and distances -> cand_off [S+1] i64, cand i32 (ascending per row, drawn from range(universe)), dist f64
    uniform in [0, 1.5 max r) with, cycling through the radii along every row's first entries: exactly float64(float32 r_j), the
    next float64 above it, +inf, 0.0."""
    rng = np.random.default_rng(seed)
    r64 = np.asarray(radii, np.float32).astype(np.float64)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cand = np.concatenate([np.sort(rng.choice(universe, c, replace=False)) for c in lengths] + [np.zeros(0, int)]).astype(np.int32)
    dist = rng.uniform(0.0, 1.5 * r64.max(), int(off[-1]))
    for i, c in enumerate(lengths):
        special = []
        for j in range(len(r64)):
            rj = r64[(i + j) % len(r64)]
            special += [rj, np.nextafter(rj, np.inf), np.inf, 0.0]
        m = min(c, len(special))
        dist[off[i]:off[i] + m] = special[:m]
    return off, cand, dist


UNI_SIZES_KEPT = (5, 6, 255, 256, 257, 1024, 1025)
UNI_SIZES_SKIPPED = (0, 4)
UNI_RADII = np.array([0.3, 0.45])
UNI_PCT = np.array([0.008, 0.012])


def uniformity_points(n=1100, seed=3):
    """n random float32 points of the unit cube; the last is a copy of the first (one coincident pair: 0 and n - 1)."""
    pts = np.random.default_rng(seed).random((n, 3)).astype(np.float32)
    pts[n - 1] = pts[0]
    return pts


def uniformity_rows(S, n=1100, seed=0):
    """S * 2 rows (seed-major, R = 2) of distinct point indices in random order.  Kept (c >= 5) and skipped (c < 5) sizes alternate
    along the seeds, in opposite phase for the two radii; at S = 65 every row of radius 1 is skipped; S = 1 holds 1025 and 5.
    The sizes cycle through UNI_SIZES_KEPT / UNI_SIZES_SKIPPED.  Rows of 1025: every other one holds the coincident pair (0, n - 1)
    at positions 0 and 1024, one in either LDS tile; the others hold neither of the two, so that the member alone in the second
    tile has a nearest other member at a distance above 0."""
    rng = np.random.default_rng(seed + S)
    rows, nk, ns, n1025 = [], 0, 0, 0
    for i in range(S):
        for j in range(2):
            keep = (i + j) % 2 == 0
            if S == 65 and j == 1:
                keep = False
            if S == 1:
                c = (1025, 5)[j]
            elif keep:
                c, nk = UNI_SIZES_KEPT[nk % len(UNI_SIZES_KEPT)], nk + 1
            else:
                c, ns = UNI_SIZES_SKIPPED[ns % len(UNI_SIZES_SKIPPED)], ns + 1
            if c == 1025:
                inner = 1 + rng.permutation(n - 2)                         # neither 0 nor n - 1
                row = np.concatenate([[0], inner[:1023], [n - 1]]) if n1025 % 2 == 0 else inner[:1025]
                n1025 += 1
            else:
                row = rng.permutation(n)[:c]
            rows.append(row.astype(np.int32))
    return rows


def _nearest_other(map_point):
    """sklearn NearestNeighbors(n_neighbors=2).kneighbors(pc, pc)[0][:, 1]: the distance to the nearest OTHER point (float64)."""
    x = np.asarray(map_point, np.float64)
    d2 = np.sum((x[:, None, :] - x[None, :, :]) ** 2, axis=-1)
    np.fill_diagonal(d2, np.inf)
    return np.sqrt(d2.min(axis=1))


def analyze_uniform(disks, radius, points, precentages=(0.008, 0.012)):
    """evaluate.py:53-101 with its file reads replaced by arguments: disks = list of index lists in `_disk_idx.txt` line order
    (seed-major, R = len(radius) per seed), radius [R], points = the projected points [n,3] (float32 as pc_util.load gives them).
    Returns uniform_measure [R] (NaN where every disk was skipped, as np.mean of an empty array)."""
    points = np.asarray(points, np.float32)
    radius = np.asarray(radius, np.float64).reshape(-1)
    precentages = np.asarray(precentages, np.float64)
    rad_number = radius.shape[0]
    sample_number = len(disks) // rad_number
    uniform_measure = np.zeros([rad_number, 1])
    densitys = np.zeros([rad_number, sample_number])
    expect_number = precentages * points.shape[0]
    expect_number = np.reshape(expect_number, [rad_number, 1])
    for j in range(rad_number):
        uniform_dis = []
        for i in range(sample_number):
            idx = list(disks[i * rad_number + j])
            densitys[j, i] = len(idx)
            coverage = np.square(densitys[j, i] - expect_number[j]) / expect_number[j]
            if len(idx) < 5:
                continue
            idx = np.array(idx).astype(np.int32)
            map_point = points[idx]
            shortest_dis = _nearest_other(map_point)
            disk_area = math.pi * (radius[j] ** 2) / map_point.shape[0]
            expect_d = math.sqrt(2 * disk_area / 1.732)
            dis = np.square(shortest_dis - expect_d) / expect_d
            dis_mean = np.mean(dis)
            uniform_dis.append(coverage * dis_mean)
        uniform_dis = np.array(uniform_dis).astype(np.float32)
        uniform_measure[j, 0] = np.mean(uniform_dis) if uniform_dis.size else np.nan
    return uniform_measure[:, 0]
