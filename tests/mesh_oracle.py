"""Float64 oracle of the evaluator's mesh metrics, for tests only (dis-pu_amd/mesh.py, csrc/mesh_eval.hip).

Written independently of the kernels: the closest point on a triangle here is the projection onto the supporting plane when it
falls inside the triangle (face region), otherwise the nearest point of the three edges as clamped segments (edge and vertex
regions); a triangle without area is its three edges.  The kernel walks Ericson's Voronoi-region tests instead.

  point_to_mesh      P2F with the best and second-best face per point (a near-tie indicator for the tolerances)
  disk_members_fp32  the membership test restated in float32: d2 = (dx*dx + dy*dy) + dz*dz <= fl32(r*r)
  analyze_uniform    evaluate.py:53-101 restated line by line, sklearn's 2-NN as the nearest other member in float64
  extract_pugan      the PU-GAN test meshes and network outputs of tests/golden/pugan_test_meshes.npz, as files
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
